// Workgroup-level fp64 product on the matrix pipe, shared by the kernels in which ONE workgroup of 256 threads owns a whole
// problem (nk_dare.hip, nk_mpc_build.hip): v_mfma_f64_16x16x4_f64 through one device function (wg_gemm), operand panels
// staged in LDS, every wave takes 16 x 16 output tiles, contraction in chunks of 16 in index order (the summation order
// depends on the sizes alone).  Device code only.
#pragma once
#include "nk_common.h"

namespace nk {

typedef double dare_d4 __attribute__((ext_vector_type(4)));

constexpr int DARE_THREADS = 256;
constexpr int DARE_ALD = 17;  // LDS row stride of the 64 x 16 panel of op(A)
constexpr int DARE_BLD = 65;  // LDS row stride of the 16 x 64 panel of op(B)

// the LDS panels of wg_gemm; a kernel's own LDS record derives from it
struct WgGemmLds {
  double As[64 * DARE_ALD];
  double Bs[16 * DARE_BLD];
};

// a matrix operand of wg_gemm: `rows` x `cols` stored entries at p (leading dimension ld), used transposed when t.
// Entries outside the stored range read as zero.
struct DareOp {
  const double* p;
  int64_t ld;
  int rows, cols;
  bool t;
};

__device__ __forceinline__ double dare_op_at(const DareOp& o, int i, int k) {  // op(o)[i][k]
  const int r = o.t ? k : i, c = o.t ? i : k;
  return (r < o.rows && c < o.cols) ? o.p[(int64_t)r * o.ld + c] : 0.0;
}

// C (Mr x Nc, leading dimension ldc; Mr, Nc multiples of 16) = / += / -= op(A) op(B), contraction length K.
// MODE 0: store, 1: add, 2: subtract.  C must not overlap the operands.  Ends with a barrier: C is visible to the workgroup.
template <int MODE>
__device__ void wg_gemm(double* C, int64_t ldc, int Mr, int Nc, int K, const DareOp A, const DareOp B, WgGemmLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;  // the wave's 32 x 32 quadrant of a 64 x 64 macro tile
  for (int i0 = 0; i0 < Mr; i0 += 64) {
    for (int j0 = 0; j0 < Nc; j0 += 64) {
      dare_d4 acc[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = dare_d4{0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < K; k0 += 16) {
        __syncthreads();  // the previous chunk's reads of As / Bs are done
        for (int e = tid; e < 64 * 16; e += DARE_THREADS) {
          int i, k;
          if (A.t) { i = e & 63; k = e >> 6; } else { k = e & 15; i = e >> 4; }  // the stored row runs fastest
          const int gi = i0 + i, gk = k0 + k;
          s.As[i * DARE_ALD + k] = (gi < Mr && gk < K) ? dare_op_at(A, gi, gk) : 0.0;
        }
        for (int e = tid; e < 16 * 64; e += DARE_THREADS) {
          int j, k;
          if (B.t) { k = e & 15; j = e >> 4; } else { j = e & 63; k = e >> 6; }
          const int gj = j0 + j, gk = k0 + k;
          // op(B)[k][j] = B.t ? B[j][k] : B[k][j]
          double v = 0.0;
          if (gj < Nc && gk < K) {
            const int r = B.t ? gj : gk, c = B.t ? gk : gj;
            if (r < B.rows && c < B.cols) v = B.p[(int64_t)r * B.ld + c];
          }
          s.Bs[k * DARE_BLD + j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int ti = wr + 16 * a, tj = wc + 16 * b;
            if (i0 + ti < Mr && j0 + tj < Nc) {  // wave-uniform
#pragma unroll
              for (int ks = 0; ks < 4; ++ks) {
                const double av = s.As[(ti + l15) * DARE_ALD + 4 * ks + l4];
                const double bv = s.Bs[(4 * ks + l4) * DARE_BLD + tj + l15];
                acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a][b], 0, 0, 0);
              }
            }
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int ti = i0 + wr + 16 * a, tj = j0 + wc + 16 * b;
          if (ti < Mr && tj < Nc) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              double* dst = C + (int64_t)(ti + l4 + 4 * reg) * ldc + tj + l15;
              if (MODE == 0) *dst = acc[a][b][reg];
              else if (MODE == 1) *dst += acc[a][b][reg];
              else *dst -= acc[a][b][reg];
            }
          }
        }
      }
    }
  }
  __syncthreads();
}

}  // namespace nk
