// Layout constants shared by the per-pose GraspReadout kernels (grasp_tail.hip: frozen weights; grasp_tail_train.hip: the training passes):
// the packed operand image mvnerf_grasp_tail_pack writes and the stash of pre-activations mvnerf_grasp_tail_fwd writes.
#pragma once

namespace mvnerf {

// ---- packed buffer (floats), K = 64 n5 ---------------------------------------------------------------------------------------------------
//   F (value, wide)  : chunk ((c * 8 + t) * 6 + nb): A[i] = (nb < 4 ? W0[32 nb + i] : Ws[32 (nb - 4) + i])[64 c + 8 t + 4 h + e]
//   V (VJP, wide)    : per offset c 48 chunks: (kt * 2 + nbo), kt < 16: A[i] = W0[8 kt + 4 h + e][64 c + 32 nbo + i]
//                                              32 + (kt * 2 + nbo), kt < 8: A[i] = Ws[8 kt + 4 h + e][64 c + 32 nbo + i]
//   C1..C3 (chain)   : W1 (4, 2), W0' (2, 2), W1' (2, 2) as dense_blocks sets, A[i][kk] = W[32 nbo + i][kk]
//   B1..B3 (chain^T) : W1'^T (2, 2), W0'^T (2, 2), W1^T (2, 4), A[i][kk] = W[kk][32 nbo + i]
//   biases           : b0 (128), b1 (64), b0' (64), b1' (64), w_out (64), b_out (1, 0 when the read-out has no bias), 3 floats of padding
constexpr int kTailStash = 320;                    // h0 | x1 | h1 | x2
constexpr int kSH0 = 0, kSX1 = 128, kSH1 = 192, kSX2 = 256;
constexpr long kWide = 64 * 192;                   // floats of F (and of V) per offset
constexpr int kC1 = 0, kC2 = kC1 + 8192, kC3 = kC2 + 4096, kB1 = kC3 + 4096, kB2 = kB1 + 4096, kB3 = kB2 + 4096, kBias = kB3 + 8192;
constexpr int kOffB0 = 0, kOffB1 = 128, kOffB0b = 192, kOffB1b = 256, kOffWout = 320, kOffBout = 384, kBiasFloats = 388;
constexpr int kSmall = kBias + kBiasFloats;        // floats behind F and V

// staging of the value-shaped kernels (one K-slice of 64 of 32 rows through LDS, A operands from L2 in a ring)
constexpr int kXs = 68;                            // LDS row stride of a staged slice (floats): 16-byte aligned rows, off the bank period
constexpr int kPre = 196;                          // LDS row stride of the 192 wide outputs
constexpr int kFwdThreads = 192;
constexpr int kAhead = 6;                          // k-steps between the request of an A operand pair and its MFMAs (ring of 8)

}  // namespace mvnerf
