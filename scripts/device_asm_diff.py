#!/usr/bin/env python3
"""Compare the kernels of two `make device-asm` trees function by function.

    python scripts/device_asm_diff.py BEFORE_DIR AFTER_DIR

For every .s file of BEFORE_DIR the bodies of its functions (label to .Lfunc_end, basic-block labels renumbered, since their
numbers count the functions in front) are compared with the same-named functions of AFTER_DIR.  Prints one line per file and
lists functions that changed, disappeared or were added.  A function that disappeared while an added one has the same body (its
own name aside) is reported as renamed - a kernel template that gained a parameter.  Exit status 1 if a function of BEFORE_DIR
changed or disappeared without such a twin."""
import os
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
            if name is None and m and not line.startswith('.'):
                name, body = m[1], []
            elif name is not None:
                if line.startswith('.Lfunc_end'):
                    # (labels and the "in Loop: Header=BB2_31" comments that name them)
                    out[name] = re.sub(r'\bBB\d+_', 'BB_', re.sub(r'\.LBB\d+_', '.LBB_', ''.join(body)))
                    name = None
                else:
                    body.append(line)
    return out


def main(before, after):
    bad = 0
    for fn in sorted(os.listdir(before)):
        if not fn.endswith('.s'):
            continue
        a = functions(os.path.join(before, fn))
        b = functions(os.path.join(after, fn)) if os.path.exists(os.path.join(after, fn)) else {}
        changed = [k for k in a if k in b and a[k] != b[k]]
        gone = [k for k in a if k not in b]
        added = [k for k in b if k not in a]
        renamed = []
        for k in list(gone):
            twin = next((n for n in added if a[k].replace(k, '@') == b[n].replace(n, '@')), None)
            if twin:
                renamed.append(f'{k} -> {twin}')
                gone.remove(k)
                added.remove(twin)
        print(f'{fn}: {len(a)} functions, {len(changed)} changed, {len(gone)} gone, {len(renamed)} renamed with the same code, {len(added)} added')
        for tag, names in (('changed', changed), ('gone', gone), ('renamed', renamed), ('added', added)):
            for k in names:
                print(f'  {tag}: {k}')
        bad += len(changed) + len(gone)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
