// The fp16 two-piece field kernel of field_eval_split16h.hip with the range guard compiled in: the same instruction stream plus a running
// maximum of |v| over every value it cuts into fp16 activation pieces, written with one atomic max per workgroup (RangeMax in
// field_eval_split16_impl.h).  Results are bit-identical to the plain kernel's; it reads the plain kernel's weight stream.
#define MVS16_F16 1
#define MVS16_GUARD 1
#include "field_eval_split16_impl.h"
