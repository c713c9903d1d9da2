// wave_ops.h — wave64 cross-lane primitives for gfx950 built on DPP row operations and the
// CDNA4 v_permlane16_swap / v_permlane32_swap instructions (all VALU, no LDS crossbar traffic;
// ds_bpermute-based __shfl costs ~10x more per step on this chip).
//
// Lane groups: a "row" is 16 lanes (DPP scope); a "half" is 32 lanes; the wave is 64.
// All functions require every lane of the participating group to be active.
#pragma once
#include <hip/hip_runtime.h>

namespace liodom_dev {

// DPP controls
constexpr int DPP_XOR1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141;  // i <-> 7-i within 8 lanes
constexpr int DPP_MIRROR = 0x140;       // i <-> 15-i within a row
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const int lo = dpp_i32<CTRL>((int)(unsigned int)v);
  const int hi = dpp_i32<CTRL>((int)(unsigned int)(v >> 32));
  return ((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  return __longlong_as_double((long long)dpp_u64<CTRL>((unsigned long long)__double_as_longlong(v)));
}

// value of the lane 16 away (same position in the neighbouring row: rows 0<->1, 2<->3)
__device__ __forceinline__ int xor16_i32(int v) {
  const auto r = __builtin_amdgcn_permlane16_swap((unsigned int)v, (unsigned int)v, false, false);
  // one result holds this lane's own row, the other the neighbouring row (rows (0,0,2,2) and
  // (1,1,3,3) of v); pick whichever differs from the own value (robust to the result order)
  const int a = (int)r[0], b = (int)r[1];
  return (a != v) ? a : b;
}
__device__ __forceinline__ int xor32_i32(int v) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned int)v, (unsigned int)v, false, false);
  const int a = (int)r[0], b = (int)r[1];   // (lo, lo) and (hi, hi) halves of v
  return (a != v) ? a : b;
}
__device__ __forceinline__ unsigned long long xor16_u64(unsigned long long v) {
  const unsigned int lo = (unsigned int)xor16_i32((int)(unsigned int)v);
  const unsigned int hi = (unsigned int)xor16_i32((int)(unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long xor32_u64(unsigned long long v) {
  const unsigned int lo = (unsigned int)xor32_i32((int)(unsigned int)v);
  const unsigned int hi = (unsigned int)xor32_i32((int)(unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// ---- max / min of u64 -------------------------------------------------------------------
__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long v) {
  unsigned long long o;
  o = dpp_u64<DPP_XOR1>(v); v = o > v ? o : v;
  o = dpp_u64<DPP_XOR2>(v); v = o > v ? o : v;
  o = dpp_u64<DPP_HALF_MIRROR>(v); v = o > v ? o : v;
  o = dpp_u64<DPP_MIRROR>(v); v = o > v ? o : v;
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = row_max_u64(v);
  unsigned long long o = xor16_u64(v); v = o > v ? o : v;
  o = xor32_u64(v); v = o > v ? o : v;
  return v;   // uniform over the wave
}
__device__ __forceinline__ unsigned long long half_min_u64(unsigned long long v) {
  unsigned long long o;
  o = dpp_u64<DPP_XOR1>(v); v = o < v ? o : v;
  o = dpp_u64<DPP_XOR2>(v); v = o < v ? o : v;
  o = dpp_u64<DPP_HALF_MIRROR>(v); v = o < v ? o : v;
  o = dpp_u64<DPP_MIRROR>(v); v = o < v ? o : v;
  o = xor16_u64(v); v = o < v ? o : v;
  return v;   // uniform over each 32-lane half
}
__device__ __forceinline__ unsigned int half_min_u32(unsigned int v) {
  unsigned int o;
  o = (unsigned int)dpp_i32<DPP_XOR1>((int)v); v = o < v ? o : v;
  o = (unsigned int)dpp_i32<DPP_XOR2>((int)v); v = o < v ? o : v;
  o = (unsigned int)dpp_i32<DPP_HALF_MIRROR>((int)v); v = o < v ? o : v;
  o = (unsigned int)dpp_i32<DPP_MIRROR>((int)v); v = o < v ? o : v;
  o = (unsigned int)xor16_i32((int)v); v = o < v ? o : v;
  return v;   // uniform over each 32-lane half
}
__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v) {
  unsigned int o;
  o = (unsigned int)dpp_i32<DPP_XOR1>((int)v); v = o > v ? o : v;
  o = (unsigned int)dpp_i32<DPP_XOR2>((int)v); v = o > v ? o : v;
  o = (unsigned int)dpp_i32<DPP_HALF_MIRROR>((int)v); v = o > v ? o : v;
  o = (unsigned int)dpp_i32<DPP_MIRROR>((int)v); v = o > v ? o : v;
  o = (unsigned int)xor16_i32((int)v); v = o > v ? o : v;
  o = (unsigned int)xor32_i32((int)v); v = o > v ? o : v;
  return v;   // uniform over the wave
}
__device__ __forceinline__ int wave_min_i32(int v) {
  int o;
  o = dpp_i32<DPP_XOR1>(v); v = o < v ? o : v;
  o = dpp_i32<DPP_XOR2>(v); v = o < v ? o : v;
  o = dpp_i32<DPP_HALF_MIRROR>(v); v = o < v ? o : v;
  o = dpp_i32<DPP_MIRROR>(v); v = o < v ? o : v;
  o = xor16_i32(v); v = o < v ? o : v;
  o = xor32_i32(v); v = o < v ? o : v;
  return v;
}

// ---- sums -------------------------------------------------------------------------------
// Sum over each 16-lane row, fixed butterfly order; every lane of the row holds the result.
__device__ __forceinline__ double row_sum_f64(double x) {
  x += dpp_f64<DPP_XOR1>(x);
  x += dpp_f64<DPP_XOR2>(x);
  x += dpp_f64<DPP_HALF_MIRROR>(x);
  x += dpp_f64<DPP_MIRROR>(x);
  return x;
}

// Reduce-scatter of a per-lane accumulator of 32 doubles over the 64 lanes of a wave (every lane active).  Halving butterfly: at
// each step a lane keeps half of its remaining entries and adds its partner's copy of that half.  Partners and the lane bit that
// picks the kept half: lane ^ 32 (v_permlane32_swap, bit 5 keeps entries 16..31), lane ^ 16 (v_permlane16_swap, bit 4), then within
// the 16-lane row r <-> 15 - r (row mirror, bit 3), r <-> 7 - r in each 8 lanes (half mirror, bit 2), r ^ 2 (bit 1); a last step
// adds the two copies of lanes r and r ^ 1.  Lane-to-entry map: lanes 2e and 2e + 1 both return the wave sum of entry e = lane >> 1
// (bit for bit: a + b == b + a).  31 + 1 FP64 adds; the pairing is fixed, so the result is deterministic.  a[] is consumed.
// v_permlane32_swap(x, y) leaves (x of lanes 0-31, y of lanes 0-31) in its first result and (x of lanes 32-63, y of lanes 32-63)
// in its second: their sum is a halving step with no select.  v_permlane16_swap does the same for odd / even 16-lane rows.
__device__ __forceinline__ double fold_xor32_f64(double x, double y) {
  const unsigned long long xb = (unsigned long long)__double_as_longlong(x), yb = (unsigned long long)__double_as_longlong(y);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned int)xb, (unsigned int)yb, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned int)(xb >> 32), (unsigned int)(yb >> 32), false, false);
  const double a = __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0]));
  const double b = __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
  return a + b;     // lanes 0-31: x + x of lane + 32; lanes 32-63: y of lane - 32 + y
}
__device__ __forceinline__ double fold_xor16_f64(double x, double y) {
  const unsigned long long xb = (unsigned long long)__double_as_longlong(x), yb = (unsigned long long)__double_as_longlong(y);
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned int)xb, (unsigned int)yb, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned int)(xb >> 32), (unsigned int)(yb >> 32), false, false);
  const double a = __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0]));
  const double b = __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
  return a + b;     // even rows: x + x of the next row; odd rows: y of the previous row + y
}
template <int CTRL>
__device__ __forceinline__ double fold_dpp_f64(double x, double y, bool upper) {
  // (the partner, which has the other `upper`, keeps what this lane gives)
  return (upper ? y : x) + dpp_f64<CTRL>(upper ? x : y);
}
__device__ __forceinline__ double wave_reduce_scatter32_f64(double (&a)[32]) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int j = 0; j < 16; j++) a[j] = fold_xor32_f64(a[j], a[j + 16]);
#pragma unroll
  for (int j = 0; j < 8; j++) a[j] = fold_xor16_f64(a[j], a[j + 8]);
#pragma unroll
  for (int j = 0; j < 4; j++) a[j] = fold_dpp_f64<DPP_MIRROR>(a[j], a[j + 4], (lane & 8) != 0);
#pragma unroll
  for (int j = 0; j < 2; j++) a[j] = fold_dpp_f64<DPP_HALF_MIRROR>(a[j], a[j + 2], (lane & 4) != 0);
  a[0] = fold_dpp_f64<DPP_XOR2>(a[0], a[1], (lane & 2) != 0);
  return a[0] + dpp_f64<DPP_XOR1>(a[0]);
}

// ---- scans ------------------------------------------------------------------------------
// Inclusive prefix sum over the wave (64 lanes).
__device__ __forceinline__ int wave_incl_scan_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR1, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR2, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR4, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR8, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST15, 0xA, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST31, 0xC, 0xF, true);
  return v;
}
// Inclusive prefix sum over each 32-lane half.
__device__ __forceinline__ int half_incl_scan_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR1, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR2, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR4, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR8, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST15, 0xA, 0xF, true);
  return v;
}

__device__ __forceinline__ int readlane_i32(int v, int lane /*wave-uniform*/) {
  return __builtin_amdgcn_readlane(v, lane);
}

}  // namespace liodom_dev
