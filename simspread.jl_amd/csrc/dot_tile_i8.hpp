// The int8 operand route of the inner-product producer (dot_csr.hip, real_floor.hip, include/simspread_hip_int8.h): the
// Gram block of one 128 x 128 tile from rows of signed 8-bit integers, on v_mfma_i32_32x32x32_i8.  The accumulator is an
// exact 32-bit integer: with d <= I8_D_MAX no sum of d products of two int8 values leaves int32, so g is THE integer
// sum_k a_k b_k whatever the order, and s of a pair is a pure function of the inputs.  After the k loop every accumulator
// register is converted to fp32 once (v_cvt_f32_i32: round to nearest even) into the f32x16 the shared epilogue expects;
// the C/D map of the instruction is Mma<float>::row of dot_tile.hpp and a wave again owns 2 x 2 MFMA tiles, so the
// epilogues of dot_tile_kernel and dot_kth_partial_kernel are shared unchanged.
//
// LAYOUT: ROW-MAJOR, element (i, k) at F[i * ld + k], ld >= d, as the 16-bit route (dot_tile_h16.hpp).  Bytes k >= d of a
// row are never interpreted and no byte past (n - 1) * ld + d - 1 is read.
//
// Staging: [TILE rows][BK8 = 128] bytes per side and step, in chunks of 16 consecutive k.  Thread t owns chunk t % 8 of
// rows t / 8 + 32 q, q = 0..3: the 8 threads of a row read its 128 contiguous bytes.  A chunk is one 16-byte load where
// that provably stays inside the row (`fast`: base 16-byte aligned and ld % 16 == 0, and k + 16 <= d), else sixteen
// guarded byte loads; k >= d and rows past n are 0.  Both ways build the same 16-byte value, so the LDS image, the MFMA
// sequence and the result do not depend on alignment or ld.
//
// LDS image: the byte image of dot_tile_h16.hpp -- row r of a side at byte 144 r (128 + one chunk of padding), chunk c at
// 144 r + 16 c, 2 x 18 KiB -- and its accesses: lane l of a 32x32x32 operand holds row l & 31, bytes k = 16 (l >> 5) + j,
// j = 0..15, i.e. one chunk, read with ds_read_b128 and staged with ds_write_b128 at the addresses of the 16-bit route.
// The conflict analysis there speaks of byte addresses only and carries over: both are conflict-free.
#pragma once
#include "dot_tile.hpp"
#include "simspread_hip_int8.h"

namespace ss {
namespace dottile {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

// operand tag of dot_tile_kernel and dot_kth_partial_kernel
struct I8 {
  using elem = int8_t;
};
// the element type in memory of an operand: T itself, or the tag's
template <class Op>
struct operand_elem {
  using type = Op;
};
template <>
struct operand_elem<I8> {
  using type = int8_t;
};

constexpr int64_t I8_D_MAX = 131071;  // d * 2^14 <= 2^31 - 1: g, A and B are exact in int32
constexpr int BK8 = 128;              // feature bytes staged per step
constexpr int LD8 = BK8 + 16;         // bytes per staged row: 144, 9 slots of 16 bytes
constexpr int CPR8 = BK8 / 16;        // chunks per row
constexpr int RPP8 = NT / CPR8;       // rows per staging pass
constexpr int NQ8 = TILE / RPP8;      // chunks per thread and side
constexpr int gram_i8_lds_bytes() { return 2 * TILE * LD8; }

// bytes k .. k + 15 of row `row` of F as one 16-byte value; 0 where k + j >= d or row >= n
__device__ __forceinline__ uint4 load_chunk_i8(const int8_t* __restrict__ F, int64_t n, int64_t ld, int64_t d, int64_t row,
                                               int64_t k, bool fast) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (row >= n || k >= d) return v;
  const int8_t* p = F + row * ld + k;
  if (fast && k + 16 <= d) return *reinterpret_cast<const uint4*>(p);  // 16-byte aligned: base, ld % 16 == 0, k % 16 == 0
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t e = k + j < d ? (uint32_t)(uint8_t)p[j] : 0u;
    w[j >> 2] |= e << (8 * (j & 3));
  }
  v.x = w[0];
  v.y = w[1];
  v.z = w[2];
  v.w = w[3];
  return v;
}

// dot_tile_gram for int8 rows: acc[i][j] = (float) of the exact Gram block of MFMA tile (i, j) of the calling wave, as
// there.  fast_a / fast_b: the side may use 16-byte loads (uniform over the grid).  Every thread of the block must call
// it.  A step is 4 k-slices of 32 x 4 MFMAs per wave; the next step's chunks are in registers during the matrix work.
__device__ __forceinline__ void dot_tile_gram_i8(const int8_t* __restrict__ Fa, int64_t na, int64_t lda,
                                                 const int8_t* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
                                                 int64_t i0, int64_t j0, bool fast_a, bool fast_b, f32x16 (&acc)[2][2]) {
  static_assert(BK8 % 32 == 0 && TILE % RPP8 == 0 && WT == 64 && NQ8 == 4, "staging shape");
  __shared__ __attribute__((aligned(16))) int8_t As[TILE][LD8];
  __shared__ __attribute__((aligned(16))) int8_t Bs[TILE][LD8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  i32x16 iacc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) iacc[i][j][r] = 0;

  const int sr = tid / CPR8, sc = (tid % CPR8) * 16;  // staging row of pass 0, first byte of the chunk
  uint4 ra[NQ8], rb[NQ8];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < NQ8; ++q) {
      ra[q] = load_chunk_i8(Fa, na, lda, d, i0 + sr + q * RPP8, k0 + sc, fast_a);
      rb[q] = load_chunk_i8(Fb, nb, ldb, d, j0 + sr + q * RPP8, k0 + sc, fast_b);
    }
  };
  if (d > 0) load(0);
  const int fr = lane & 31, fk = 16 * (lane >> 5);
  for (int64_t k0 = 0; k0 < d; k0 += BK8) {
#pragma unroll
    for (int q = 0; q < NQ8; ++q) {
      *reinterpret_cast<uint4*>(&As[sr + q * RPP8][sc]) = ra[q];
      *reinterpret_cast<uint4*>(&Bs[sr + q * RPP8][sc]) = rb[q];
    }
    __syncthreads();
    if (k0 + BK8 < d) load(k0 + BK8);  // the next step's loads are in flight during this step's matrix work
#pragma unroll
    for (int kk = 0; kk < BK8; kk += 32) {
      i32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const i32x4*>(&As[wm * WT + i * 32 + fr][kk + fk]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const i32x4*>(&Bs[wn * WT + j * 32 + fr][kk + fk]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          iacc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], iacc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = (float)iacc[i][j][r];  // one conversion, round to nearest even
}

// N[i] = (float) sum_k F[i, k]^2, the sum exact in int32.  16 lanes per row: lane j takes k = j, j + 16, ..., then a xor
// tree over the 16 partial sums (integer: the order does not matter).
static __global__ void row_norm_i8_kernel(const int8_t* __restrict__ F, int64_t n, int64_t ld, int64_t d,
                                          float* __restrict__ N) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int j = threadIdx.x & 15;
  int s = 0;
  if (i < n) {
    const int8_t* p = F + i * ld;
    for (int64_t k = j; k < d; k += 16) {
      const int x = p[k];
      s += x * x;
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (i < n && j == 0) N[i] = (float)s;
}

}  // namespace dottile
}  // namespace ss
