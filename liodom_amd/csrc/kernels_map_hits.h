// Per-scan map-hit records of reader streams (liodom_set_map_hits / liodom_map_hit_rows; no counterpart in the reference): the two
// counts liodom_map_score_poses defines, one row = one edge cloud under one pose.  Included at the end of liodom_map.h, after
// kernels_reloc.h, whose contract it keeps to the bit: reloc_axis, reloc_find, reloc_bit and transform_point are used as they
// stand, and an edge is tested exactly as k_map_score_poses tests it (probes, keys, leaf test, finiteness rules).
// Nothing of the map is written; the occupancy is the map's own buffer, built by k_map_occ_clear + k_map_occ_build before the
// launch (liodom_map_host.h keeps it while the map's generation stands).
#pragma once

namespace liodom_dev {

constexpr int kMapHitThreads = 256;
constexpr int kMapHitWaves = kMapHitThreads / 64;
constexpr int kMapHitRecordBytes = 128;                // sizeof(liodom_map_hit_t)
constexpr unsigned int kMapHitValid = 1u, kMapHitNoReader = 2u, kMapHitNoSolve = 4u;      // LIODOM_HIT_*

// Where the rows of a launch live, in the scheme of MapRows: row `row` works for idx = s0 + row, or list[row] (kList).
//   batch call (log == nullptr): every row takes part with `radius`; hits[2 idx], hits[2 idx + 1] = hits_r, hits_0.
//   step path (log != nullptr): idx is a stream.  It takes part iff radius_of[idx] >= 0 and the tag of the map it reads
//     (sel[idx].x; 0 without a reader, and for every stream while sel == nullptr) equals `tag`.  tag > 0: the stream's scan is
//     counted against THIS map and gets a VALID record; tag == 0: it gets a NO_READER record, and the map is not looked at.
//     The record goes to entry scan_no[idx] - 1 of the stream's log (the scan's liodom_step_info_t.scan_index: finalize_scan has
//     counted the scan by now); an entry at or beyond log_cap is not written, as in the pose log.
struct MapHitRows {
  const float4* edges; long long edge_stride;      // cloud of idx: edges + idx * edge_stride
  const int* n_edges;  long long n_stride;         // its points: n_edges[idx * n_stride], clamped to 0 .. edge_cap
  const double* T;     long long T_stride;         // pose of idx: T + idx * T_stride, 12 doubles (row-major 3 x 4)
  int edge_cap, radius;
  int* hits;
  uint4* log; int log_cap;                         // [stream][log_cap] records of kMapHitRecordBytes
  const int* scan_no; const int* raw;              // StreamState::scan_counter / append_raw of idx, strided as n_edges
  const int* radius_of; const int4* sel; const int* list;
  int tag, s0;
};

// one edge under T, as the body of k_map_score_poses' loop has it
__device__ __forceinline__ void map_hit_edge(const MapView& m, const unsigned int* __restrict__ occ, int occ_cells, const double* T, const float4 e,
                                             int radius, float leaf, bool* h0_out, bool* hr_out) {
  float qx, qy, qz;
  transform_point(T, e.x, e.y, e.z, &qx, &qy, &qz);
  const RelocAxis ax = reloc_axis(qx, leaf, m.leaf_inv, m.inv_xy, m.xy, m.half_xy);
  const RelocAxis ay = reloc_axis(qy, leaf, m.leaf_inv, m.inv_xy, m.xy, m.half_xy);
  const RelocAxis az = reloc_axis(qz, leaf, m.leaf_inv, m.inv_z, m.z, m.half_z);
  bool h0 = false;
  int c0 = -1;
  if (ax.fin[1] && ay.fin[1] && az.fin[1]) c0 = reloc_find(m, occ_cells, ax.key[1], ay.key[1], az.key[1]);
  if (c0 >= 0) h0 = reloc_bit(m, occ, c0, ax.leaf[1], ay.leaf[1], az.leaf[1]);
  bool hr = h0;
  if (radius && !hr) {
    for (int k = 0; k < 27 && !hr; k++) {
      if (k == 13) continue;                    // the centre
      const int jx = k % 3, jy = (k / 3) % 3, jz = k / 9;
      if (!(reloc_sel3(jx, ax.fin[0], ax.fin[1], ax.fin[2]) && reloc_sel3(jy, ay.fin[0], ay.fin[1], ay.fin[2]) &&
            reloc_sel3(jz, az.fin[0], az.fin[1], az.fin[2]))) continue;
      const int kx = reloc_sel3(jx, ax.key[0], ax.key[1], ax.key[2]), ky = reloc_sel3(jy, ay.key[0], ay.key[1], ay.key[2]),
                kz = reloc_sel3(jz, az.key[0], az.key[1], az.key[2]);
      const int cell = (kx == ax.key[1] && ky == ay.key[1] && kz == az.key[1]) ? c0 : reloc_find(m, occ_cells, kx, ky, kz);
      if (cell < 0) continue;
      hr = reloc_bit(m, occ, cell, reloc_sel3(jx, ax.leaf[0], ax.leaf[1], ax.leaf[2]), reloc_sel3(jy, ay.leaf[0], ay.leaf[1], ay.leaf[2]),
                     reloc_sel3(jz, az.leaf[0], az.leaf[1], az.leaf[2]));
    }
  }
  *h0_out = h0; *hr_out = hr;
}

// One 256-thread workgroup per row (a 64 x 1800 scan has up to 5120 edges: 80 dependent rounds for one wave, 20 here).
//   row        everything that selects the row and its pose depends on blockIdx alone: the stream, its radius, tag, edge count
//              and the pose's 12 doubles are wave-uniform loads
//   edges      one 16-byte load per lane and edge through the cache, the four waves stride the rounds of 64 edges
//   counts     ballot + popcount per round, summed in scalar registers; the waves combine through four LDS words (two counts
//              each) and one barrier.  No global atomics.
//   output     thread 0 alone: the 128-byte record as eight 16-byte vector stores, or the batch form's pair as one 8-byte store
template <bool kList = false>
__global__ __launch_bounds__(kMapHitThreads) void k_map_hit_rows(MapView m, const unsigned int* __restrict__ occ, int occ_cells, float leaf, MapHitRows r) {
  __shared__ int2 sh_cnt[kMapHitWaves];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int row = blockIdx.x;
  const int idx = kList ? r.list[row] : r.s0 + row;
  int radius = r.radius;
  int k = 0;
  bool counted = true;
  if (r.log) {                                    // (everything here is uniform over the workgroup)
    radius = r.radius_of[idx];
    if (radius < 0) return;                       // hits are off for this stream
    if ((r.sel ? r.sel[idx].x : 0) != r.tag) return;      // another map's reader (or, with tag 0, a reader)
    k = r.scan_no[(long long)idx * r.n_stride] - 1;
    if (k < 0 || k >= r.log_cap) return;          // beyond the log, as the pose log
    counted = r.tag > 0;
  }
  const double* Tp = r.T + (long long)idx * r.T_stride;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = Tp[i];
  int n = 0, n_r = 0, n_0 = 0;
  if (counted) {
    n = max(0, min(r.n_edges[(long long)idx * r.n_stride], r.edge_cap));
    const float4* edges = r.edges + (long long)idx * r.edge_stride;
    for (int base = wave * 64; base < n; base += kMapHitThreads) {
      const int i = base + lane;
      bool h0 = false, hr = false;
      if (i < n) map_hit_edge(m, occ, occ_cells, T, edges[i], radius, leaf, &h0, &hr);
      n_r += __popcll(__ballot(hr));
      n_0 += __popcll(__ballot(h0));
    }
  }
  if (lane == 0) sh_cnt[wave] = make_int2(n_r, n_0);
  __syncthreads();
  if (tid != 0) return;
  int hits_r = 0, hits_0 = 0;
#pragma unroll
  for (int w = 0; w < kMapHitWaves; w++) { hits_r += sh_cnt[w].x; hits_0 += sh_cnt[w].y; }
  if (!r.log) { reinterpret_cast<int2*>(r.hits)[idx] = make_int2(hits_r, hits_0); return; }
  unsigned int flags = counted ? kMapHitValid : kMapHitNoReader;
  if (r.raw[(long long)idx * r.n_stride]) flags |= kMapHitNoSolve;      // the scan was its stream's first and did not solve
  uint4* rec = r.log + ((size_t)idx * (size_t)r.log_cap + (size_t)k) * (kMapHitRecordBytes / 16);
  rec[0] = make_uint4((unsigned int)k, flags, (unsigned int)n, (unsigned int)hits_r);
  rec[1] = make_uint4((unsigned int)hits_0, (unsigned int)radius, 0u, 0u);
  double2* rt = reinterpret_cast<double2*>(rec + 2);
#pragma unroll
  for (int i = 0; i < 6; i++) rt[i] = make_double2(T[2 * i], T[2 * i + 1]);
}

}  // namespace liodom_dev
