// The 16-bit operand route of the inner-product producer (dot_csr.hip, include/simspread_hip_half.h): the Gram block of
// one 128 x 128 tile from rows stored as raw bf16 / fp16 bit patterns, on v_mfma_f32_32x32x16_{bf16,f16}.  Every product
// of two 16-bit values is exact in fp32 and the accumulator is fp32, so nothing the fp32 route keeps is lost; only the
// order of the sums is the instruction's.  The C/D map of the instruction is Mma<float>::row of dot_tile.hpp and a wave
// again owns 2 x 2 MFMA tiles in 64 accumulator registers, so the epilogue of dot_tile_kernel is shared unchanged.
//
// LAYOUT: ROW-MAJOR, element (i, k) at F[i * ld + k], ld >= d -- unlike the column-major fp32 / fp64 operands of
// dot_tile.hpp.  Elements k >= d of a row are never interpreted and no byte past element (n - 1) * ld + d - 1 is read.
//
// Staging: [TILE rows][BK16 = 64] elements per side and step, in chunks of 8 consecutive k (16 bytes).  Thread t owns
// chunk t % 8 of rows t / 8 + 32 q, q = 0..3: the 8 threads of a row read its 128 contiguous bytes.  A chunk is one
// 16-byte load where that provably stays inside the row (`fast`: base 16-byte aligned and ld % 8 == 0, and k + 8 <= d),
// else eight guarded 2-byte loads; k >= d and rows past n are 0.  Both ways build the same 16-byte value, so the LDS
// image, the MFMA sequence and the result bits do not depend on alignment or ld.
//
// LDS image: row r of a side at byte 144 r (LDH = 72 elements: 64 + one chunk of padding), chunk c at 144 r + 16 c.
//   ds_read_b128 (fragments): banks are (a / 4) % 64, i.e. 16 slots of 16 bytes, served in four groups of 16 lanes that
//   lie in one half wave ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32).  A group's lanes read one chunk
//   column of 16 rows whose indices are pairwise distinct mod 16; row r sits on slot (9 r + c) % 16 and 9 is odd, so
//   the 16 slots are distinct: conflict-free.
//   ds_write_b128 (staging): banks are (a / 4) % 32, served in groups of 8 consecutive lanes = the 8 chunks of one row =
//   128 contiguous bytes = 32 distinct banks: conflict-free.
#pragma once
#include "dot_tile.hpp"
#include "simspread_hip_half.h"

namespace ss {
namespace dottile {

// operand tags of dot_tile_kernel: the element type in memory and the matrix instruction
struct Bf16 {
  using elem = uint16_t;
  using frag = __attribute__((ext_vector_type(8))) __bf16;
  static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __host__ __device__ __forceinline__ bool is_nan(uint16_t x) { return (x & 0x7fffu) > 0x7f80u; }
  static __device__ __forceinline__ float widen(uint16_t x) { return __uint_as_float((uint32_t)x << 16); }
};
struct F16 {
  using elem = uint16_t;
  using frag = __attribute__((ext_vector_type(8))) _Float16;
  static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __host__ __device__ __forceinline__ bool is_nan(uint16_t x) { return (x & 0x7fffu) > 0x7c00u; }
  static __device__ __forceinline__ float widen(uint16_t x) {
    union { uint16_t u; _Float16 h; } c;
    c.u = x;
    return (float)c.h;  // exact
  }
};

constexpr int BK16 = 64;       // feature columns staged per step
constexpr int LDH = BK16 + 8;  // elements per staged row: 144 bytes, 9 slots of 16 bytes (see the header comment)
constexpr int CPR = BK16 / 8;  // chunks per row
constexpr int RPP = NT / CPR;  // rows per staging pass
constexpr int NQ = TILE / RPP; // chunks per thread and side

// 8 consecutive elements k .. k + 7 of row `row` of F as one 16-byte value; 0 where k + j >= d or row >= n
__device__ __forceinline__ uint4 load_chunk_h16(const uint16_t* __restrict__ F, int64_t n, int64_t ld, int64_t d,
                                                int64_t row, int64_t k, bool fast) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (row >= n || k >= d) return v;
  const uint16_t* p = F + row * ld + k;
  if (fast && k + 8 <= d) return *reinterpret_cast<const uint4*>(p);  // 16-byte aligned: base, ld % 8 == 0, k % 8 == 0
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = k + j < d ? (uint32_t)p[j] : 0u;
  v.x = e[0] | (e[1] << 16);
  v.y = e[2] | (e[3] << 16);
  v.z = e[4] | (e[5] << 16);
  v.w = e[6] | (e[7] << 16);
  return v;
}

// dot_tile_gram for 16-bit rows: acc[i][j] = the Gram block of MFMA tile (i, j) of the calling wave, as there.
// fast_a / fast_b: the side may use 16-byte loads (uniform over the grid).  Every thread of the block must call it.
// Lane l of a 32x32x16 operand holds row l & 31, k = 8 (l >> 5) + j, j = 0..7: one chunk of the staged image.
template <class Op>
__device__ __forceinline__ void dot_tile_gram_h16(const uint16_t* __restrict__ Fa, int64_t na, int64_t lda,
                                                  const uint16_t* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
                                                  int64_t i0, int64_t j0, bool fast_a, bool fast_b,
                                                  f32x16 (&acc)[2][2]) {
  static_assert(BK16 % 16 == 0 && TILE % RPP == 0 && WT == 64, "staging shape");
  __shared__ __attribute__((aligned(16))) uint16_t As[TILE][LDH];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[TILE][LDH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int sr = tid / CPR, sc = (tid % CPR) * 8;  // staging row of pass 0, first element of the chunk
  uint4 ra[NQ], rb[NQ];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      ra[q] = load_chunk_h16(Fa, na, lda, d, i0 + sr + q * RPP, k0 + sc, fast_a);
      rb[q] = load_chunk_h16(Fb, nb, ldb, d, j0 + sr + q * RPP, k0 + sc, fast_b);
    }
  };
  if (d > 0) load(0);
  const int fr = lane & 31, fk = 8 * (lane >> 5);
  for (int64_t k0 = 0; k0 < d; k0 += BK16) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      *reinterpret_cast<uint4*>(&As[sr + q * RPP][sc]) = ra[q];
      *reinterpret_cast<uint4*>(&Bs[sr + q * RPP][sc]) = rb[q];
    }
    __syncthreads();
    if (k0 + BK16 < d) load(k0 + BK16);  // the next step's loads are in flight during this step's matrix work
#pragma unroll
    for (int kk = 0; kk < BK16; kk += 16) {
      typename Op::frag av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        av[i] = *reinterpret_cast<const typename Op::frag*>(&As[wm * WT + i * 32 + fr][kk + fk]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bv[j] = *reinterpret_cast<const typename Op::frag*>(&Bs[wn * WT + j * 32 + fr][kk + fk]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Op::mma(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
}

// N[i] = sum_k w(F[i, k])^2 in fp32, every square exact.  16 lanes per row: lane j takes k = j, j + 16, ... in order, then
// a xor tree over the 16 partial sums: an order that depends on d alone, not on ld or the alignment of F.
template <class Op>
static __global__ void row_norm_h16_kernel(const uint16_t* __restrict__ F, int64_t n, int64_t ld, int64_t d,
                                           float* __restrict__ N) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int j = threadIdx.x & 15;
  float s = 0.0f;
  if (i < n) {
    const uint16_t* p = F + i * ld;
    for (int64_t k = j; k < d; k += 16) {
      const float x = Op::widen(p[k]);
      s += x * x;
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (i < n && j == 0) N[i] = s;
}

// *flag = 1 when an element k < d of a row of F is a NaN pattern of the storage format
template <class Op>
static __global__ void nan_scan_h16_kernel(const uint16_t* __restrict__ F, int64_t n, int64_t ld, int64_t d,
                                           int* __restrict__ flag) {
  // 16 lanes per row, as row_norm_h16_kernel: lane j looks at k = j, j + 16, ... < d; the groups stride over the rows
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> 4;
  const int j = threadIdx.x & 15;
  bool bad = false;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; i < n; i += groups) {
    const uint16_t* p = F + i * ld;
    for (int64_t k = j; k < d; k += 16) bad |= Op::is_nan(p[k]);
  }
  if (bad) *flag = 1;
}

}  // namespace dottile
}  // namespace ss
