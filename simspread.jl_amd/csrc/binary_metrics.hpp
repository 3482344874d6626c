// The six confusion-matrix metrics of the reference (f1score, mcc, accuracy, balancedaccuracy, recall, precision;
// src/performance.jl:102-296) at one threshold, as the host mirror (simspread.jl_amd/metrics.py) evaluates them on
// integer counts: in double, operation for operation, without FP contraction.  Shared by the per-row binary metrics
// (binary_rows.hip) and the pooled tables (pooled.hip), so that both give one value for one set of counts.
//
// mcc's numerator tp*tn - fp*fn and its denominator p_pred*n_pred*p_act*n_act are the mirror's Python integers: the
// numerator is formed in 128 bits, the denominator's two halves too, and each integer is rounded to double once
// (round to nearest even), so the counts may exceed 2^31 (pooled sweeps reach 10^10 and more).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

__device__ inline double br_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// mcc(a, b, eps) limit form (metrics.py): (a*e - b*e) / sqrt((a+b)*(a+e)*(b+e)*(e+e)), e = floatmin(Float64)
__device__ inline double br_mcc_limit(long long ai, long long bi) {
#pragma clang fp contract(off)
  const double a = (double)ai, b = (double)bi, e = 2.2250738585072014e-308;
  return (a * e - b * e) / sqrt((a + b) * (a + e) * (b + e) * (e + e));
}

// the double nearest to the unsigned integer sum_k r[k] 2^(64k) (ties to even): the top 64 significant bits with
// every lower bit folded into a sticky bit, converted once (53 < 63 bits, so the sticky bit decides only ties)
__device__ inline double br_limbs_to_double(const uint64_t* r, int nl) {
  int k = nl - 1;
  while (k > 0 && r[k] == 0) --k;
  if (k == 0) return (double)r[0];
  const int lz = __clzll(r[k]);
  uint64_t top = r[k], lost = r[k - 1];
  if (lz) {
    top = (r[k] << lz) | (r[k - 1] >> (64 - lz));
    lost = r[k - 1] << lz;
  }
  for (int j = 0; j < k - 1; ++j) lost |= r[j];
  return ldexp((double)(top | (lost != 0 ? 1ULL : 0ULL)), 64 * k - lz);
}

__device__ inline double br_u128_to_double(unsigned __int128 v) {
  const uint64_t r[2] = {(uint64_t)v, (uint64_t)(v >> 64)};
  return br_limbs_to_double(r, 2);
}

// double(a * b) for the exact 256-bit product of two 128-bit integers
__device__ inline double br_mul_to_double(unsigned __int128 a, unsigned __int128 b) {
  const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
  const unsigned __int128 p00 = (unsigned __int128)a0 * b0, p01 = (unsigned __int128)a0 * b1,
                          p10 = (unsigned __int128)a1 * b0, p11 = (unsigned __int128)a1 * b1;
  uint64_t r[4];
  r[0] = (uint64_t)p00;
  unsigned __int128 m = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;  // < 3 * 2^64
  r[1] = (uint64_t)m;
  m = (m >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t)p11;
  r[2] = (uint64_t)m;
  r[3] = (uint64_t)((m >> 64) + (p11 >> 64));
  return br_limbs_to_double(r, 4);
}

// the six metrics at one threshold, as metrics.py evaluates them on integer counts
__device__ inline void br_metrics(long long tp, long long fp, long long P, long long N, double* m) {
#pragma clang fp contract(off)
  const long long tn = N - fp, fn = P - tp;
  const double d = (double)tp + 0.5 * (double)(fp + fn);
  m[0] = d == 0.0 ? br_nan() : (double)tp / d;
  const long long p_pred = tp + fp, n_pred = fn + tn, p_act = tp + fn, n_act = fp + tn;
  if (p_pred == 0) m[1] = br_mcc_limit(tn, fn);
  else if (n_pred == 0) m[1] = br_mcc_limit(tp, fp);
  else if (p_act == 0) m[1] = br_mcc_limit(tn, fp);
  else if (n_act == 0) m[1] = br_mcc_limit(tp, fn);
  else {
    const __int128 num = (__int128)tp * tn - (__int128)fp * fn;
    const double num_d = num < 0 ? -br_u128_to_double((unsigned __int128)(-num)) : br_u128_to_double((unsigned __int128)num);
    const unsigned __int128 a = (unsigned __int128)p_pred * (unsigned __int128)n_pred,
                            b = (unsigned __int128)p_act * (unsigned __int128)n_act;
    // below 2^53 both halves are exact doubles and one rounded product is the exact product rounded once
    const double den = (a >> 53) == 0 && (b >> 53) == 0 ? (double)(uint64_t)a * (double)(uint64_t)b
                                                        : br_mul_to_double(a, b);
    m[1] = num_d / sqrt(den);
  }
  m[2] = (double)(tp + tn) / (double)((tp + tn) + (fp + fn));
  const double tpr = p_act != 0 ? (double)tp / (double)p_act : br_nan();
  const double tnr = n_act != 0 ? (double)tn / (double)n_act : br_nan();
  m[3] = (tpr + tnr) / 2.0;
  m[4] = p_act == 0 ? br_nan() : (double)tp / (double)p_act;
  m[5] = p_pred == 0 ? br_nan() : (double)tp / (double)p_pred;
}

}  // namespace ss
