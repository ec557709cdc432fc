// gs_features.hip -- per-Gaussian feature channels rendered through one view's tile lists (gfx950).
//
// With "composited", alpha_i(p), T_i(p) and the T recurrence those of the colour forward of the
// numerics mode (gs_contrib.hip, gs_contrib_stats in gsrast.h) and features f [P, C]:
//   forward    out[c, p] = sum_i f_i[c] alpha_i(p) T_i(p)          every channel composited in the
//              form and order of a colour channel (exact: acc + (f alpha) T, fast: fma(f, alpha T,
//              acc), list order); no background term, f is not clamped
//   backward   dL/df_i[c] = sum_p alpha_i(p) T_i(p) g_c(p)         gs_contrib_stats' wsum with the
//              weight map replaced by channel c of the image gradient
// The geometry is constant: nothing here differentiates alpha or T.  Channels run in groups of
// FEAT_G per walk; the walks are gs_contrib.hip's (one wave per tile, four pixel slots per lane,
// 64-entry batches staged in LDS with the per-quadrant cull, front to back from T = 1):
//   k_feature_fwd       the group's FEAT_G floats of each staged entry's feature row are staged
//                       beside its splat coefficients; 4 slots x FEAT_G accumulators per lane
//   k_feature_bwd_walk  g[c, p] of the group held per slot; per walked entry FEAT_G wave sums of
//                       g_c w and one FEAT_G-float record per (tile, Gaussian) instance
//   k_feature_sum       k_contrib_sum with FEAT_G sums: per Gaussian over its slot range in fp64,
//                       rounded once, written (or added) to the group's columns of its row
// No float atomics on global memory and a fixed order everywhere: bitwise reproducible.
#include "gs_internal.h"

namespace gs {

constexpr int FEAT_G = GS_FEATURE_GROUP;
static_assert(FEAT_G == 8, "the staged rows and the records are two float4 per entry");

struct FeatSlot {
  float T;        // transmittance in front of the next entry
  uint32_t last;  // n_contrib of the pixel (0 outside the image)
};

// one slot's alpha for one entry (0 where the entry is not composited: T passes through bit for
// bit) -- the decision of contrib_slot; sets con where it is composited
template <bool EXACT>
__device__ __forceinline__ float feat_alpha(const FeatSlot& q, float pfx, float pfy, const float2 xy, const float4 co,
                                            uint32_t e, bool& con) {
  const float dx = xy.x - pfx, dy = xy.y - pfy;
  const float pw = falloff_log2_m<EXACT>(co, dx, dy);  // log2(e) * power (fast: + log2 o)
  const float oG = opac_gauss<EXACT>(co, pw);
  con = e < q.last && (!EXACT || pw <= 0.0f) && oG >= 1.0f / 255.0f;
  return con ? fminf(0.99f, oG) : 0.0f;
}
template <bool EXACT>
__device__ __forceinline__ void feat_step_T(FeatSlot& q, float a) {
  if constexpr (EXACT)
    q.T = q.T * (1.0f - a);
  else
    q.T = __builtin_fmaf(-a, q.T, q.T);
}

// the group's FEAT_G floats of row gid (zeros past the row's end: the tail group)
__device__ __forceinline__ void feat_load_row(const float* __restrict__ features, uint32_t gid, int C, int c0,
                                              float (&f)[FEAT_G]) {
  const float* row = features + (size_t)gid * (size_t)C + c0;
#pragma unroll
  for (int k = 0; k < FEAT_G; k++) f[k] = c0 + k < C ? row[k] : 0.0f;
}

// the staging pipeline shared by the two walks (one entry per lane, as in k_contrib_walk): while
// batch k is walked, the splat records of batch k + 1, the ids of batch k + 2 and the slots of batch
// k + 3 are in flight; entries past the walk's end are clamped to its last one.
struct FeatTile {
  uint32_t tile, n_eff;
  uint32_t qlast[4];
  uint2 range;
  int tx, ty;
};
__device__ __forceinline__ bool feat_tile(const CameraArgs& c, const uint2* __restrict__ ranges,
                                          const uint32_t* __restrict__ tile_max, uint32_t tile, bool invalid,
                                          FeatTile& t) {
  t.tile = tile;
  t.tx = (int)(tile % (uint32_t)c.gx), t.ty = (int)(tile / (uint32_t)c.gx);
  t.range = ranges[tile];
  const uint32_t n = invalid ? 0u : t.range.y - t.range.x;
  // per-quadrant largest n_contrib (the forward's quadrant waves): slot k's walk ends there
  const uint4 qm = reinterpret_cast<const uint4*>(tile_max)[tile];
  t.qlast[0] = min(qm.x, n), t.qlast[1] = min(qm.y, n), t.qlast[2] = min(qm.z, n), t.qlast[3] = min(qm.w, n);
  t.n_eff = max(max(t.qlast[0], t.qlast[1]), max(t.qlast[2], t.qlast[3]));
  return t.n_eff != 0;
}

// ------------------------------------------------------------------------------------------
// forward: grid (tiles, channel groups)
// ------------------------------------------------------------------------------------------
template <bool EXACT>
__global__ __launch_bounds__(64) void k_feature_fwd(CameraArgs c, const uint2* __restrict__ ranges,
                                                    const uint32_t* __restrict__ point_list,
                                                    const uint32_t* __restrict__ point_gid,
                                                    const float4* __restrict__ splat,
                                                    const uint32_t* __restrict__ n_contrib,
                                                    const uint32_t* __restrict__ tile_max,
                                                    const uint32_t* __restrict__ tile_order,
                                                    const uint32_t* __restrict__ err,
                                                    const float* __restrict__ features, int C,
                                                    float* __restrict__ out) {
  __shared__ float2 s_xy[64];
  __shared__ float4 s_co[64];     // falloff coefficients + opacity (fall_coefs)
  __shared__ float4 s_f[64][2];   // the group's FEAT_G features of the batch's entries
  const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_order[blockIdx.x]);
  if (tile == ~0u) return;  // a hole of the XCD-group launch order
  const int c0 = (int)blockIdx.y * FEAT_G;
  const int lane = threadIdx.x;
  FeatTile t;
  // a view whose forward recorded an invalid instance list has no valid list: zeros
  const bool walk = feat_tile(c, ranges, tile_max, tile, (*err & ERR_INVALID) != 0, t);
  const int tx = t.tx, ty = t.ty;

  const int qx0 = tx * GS_TILE + (lane & 7), qy0 = ty * GS_TILE + (lane >> 3);
  FeatSlot p[4];
  float acc[4][FEAT_G];
  bool in[4];
  size_t pixk[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int px = qx0 + 8 * (k & 1), py = qy0 + 8 * (k >> 1);
    in[k] = px < c.W && py < c.H;
    pixk[k] = in[k] ? (size_t)py * c.W + px : 0;
    p[k].T = 1.0f;
    p[k].last = in[k] && walk ? n_contrib[pixk[k]] : 0u;
#pragma unroll
    for (int ch = 0; ch < FEAT_G; ch++) acc[k][ch] = 0.0f;
  }
  const float pfx0 = (float)qx0, pfy0 = (float)qy0;

  if (walk) {
    const uint32_t n_eff = t.n_eff;
    const uint32_t e_last = n_eff - 1;
    const uint32_t* const plist = point_list + t.range.x;
    auto pos = [&](uint32_t e) { return min(e, e_last); };
    uint32_t G1 = point_gid[plist[pos((uint32_t)lane)]];
    float4 pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
    float fr[FEAT_G];
    feat_load_row(features, G1, C, c0, fr);
    uint32_t S1 = plist[pos((uint32_t)lane + 64u)];
    G1 = point_gid[S1];
    uint32_t S2 = plist[pos((uint32_t)lane + 128u)];

    for (uint32_t base = 0; base < n_eff; base += 64) {
      const uint32_t cnt = min(64u, n_eff - base);
      const bool mine = (uint32_t)lane < cnt;
      uint32_t qmask = 0;
      if (mine) {
        s_xy[lane] = make_float2(pa.x, pa.y);
        s_co[lane] = fall_coefs_m<EXACT>(pa.z, pa.w, pb.x, pb.y);
        s_f[lane][0] = make_float4(fr[0], fr[1], fr[2], fr[3]);
        s_f[lane][1] = make_float4(fr[4], fr[5], fr[6], fr[7]);
        qmask = quadrant_mask(pa.x, pa.y, pa.z, pa.w, pb.x, pd.z, tx, ty);
      }
      // issue the next batch's splat and feature loads, the ids after it and the slots after those
      pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
      feat_load_row(features, G1, C, c0, fr);
      S1 = S2;
      G1 = point_gid[S2];
      S2 = plist[pos(base + 192u + (uint32_t)lane)];
      // per-slot entry sets: entry j of the batch reaches quadrant k iff base + j < qlast[k]
      uint64_t M[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint64_t mk = __ballot((qmask >> k) & 1u);
        const uint32_t jn = t.qlast[k] > base ? t.qlast[k] - base : 0u;
        if (jn < 64u) mk &= (1ull << jn) - 1ull;
        M[k] = mk;
      }
      __builtin_amdgcn_wave_barrier();
      uint64_t m = (M[0] | M[1]) | (M[2] | M[3]);
#pragma unroll 1
      while (m) {
        const uint32_t j = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const float2 xy = s_xy[j];
        const float4 co = s_co[j];
        const float4 f0 = s_f[j][0], f1 = s_f[j][1];
        const float f[FEAT_G] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
        const uint32_t e = base + j;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if ((M[k] >> j) & 1ull) {
            bool con;
            const float a =
                feat_alpha<EXACT>(p[k], pfx0 + (float)(8 * (k & 1)), pfy0 + (float)(8 * (k >> 1)), xy, co, e, con);
            if constexpr (EXACT) {
              // (f alpha) T, a colour channel's form; a pixel where the entry is not composited keeps
              // its sums (the forward's select)
#pragma unroll
              for (int ch = 0; ch < FEAT_G; ch++) acc[k][ch] = con ? acc[k][ch] + f[ch] * a * p[k].T : acc[k][ch];
            } else {
              const float w = a * p[k].T;  // 0 where not composited, as the forward's weight
#pragma unroll
              for (int ch = 0; ch < FEAT_G; ch++) acc[k][ch] = __builtin_fmaf(f[ch], w, acc[k][ch]);
            }
            feat_step_T<EXACT>(p[k], a);
          }
      }
      __builtin_amdgcn_wave_barrier();  // the next batch overwrites the staged entries
    }
  }
  // every pixel of the image is written (zeros in a tile without a walked entry)
  const size_t HW = (size_t)c.W * c.H;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (in[k]) {
#pragma unroll
      for (int ch = 0; ch < FEAT_G; ch++)
        if (c0 + ch < C) out[(size_t)(c0 + ch) * HW + pixk[k]] = acc[k][ch];
    }
}

// ------------------------------------------------------------------------------------------
// backward walk: one record of FEAT_G floats per (tile, Gaussian) instance
// ------------------------------------------------------------------------------------------
template <bool EXACT>
__global__ __launch_bounds__(64) void k_feature_bwd_walk(CameraArgs c, const uint2* __restrict__ ranges,
                                                         const uint32_t* __restrict__ point_list,
                                                         const uint32_t* __restrict__ point_gid,
                                                         const float4* __restrict__ splat,
                                                         const uint32_t* __restrict__ n_contrib,
                                                         const uint32_t* __restrict__ tile_max,
                                                         const uint32_t* __restrict__ tile_order,
                                                         const float* __restrict__ dL_dout, int C, int c0,
                                                         float4* __restrict__ rec) {
  __shared__ float2 s_xy[64];
  __shared__ float4 s_co[64];
  __shared__ float4 s_rec[64][2];  // the FEAT_G sums of the batch's entries
  const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_order[blockIdx.x]);
  if (tile == ~0u) return;  // a hole of the XCD-group launch order
  const int lane = threadIdx.x;
  FeatTile t;
  if (!feat_tile(c, ranges, tile_max, tile, false, t)) return;  // no instance walked: no records
  const int tx = t.tx, ty = t.ty;
  const uint32_t n_eff = t.n_eff;

  const int qx0 = tx * GS_TILE + (lane & 7), qy0 = ty * GS_TILE + (lane >> 3);
  const size_t HW = (size_t)c.W * c.H;
  FeatSlot p[4];
  float g[4][FEAT_G];  // the group's image gradient at the slot's pixel (0 outside the image / the row)
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int px = qx0 + 8 * (k & 1), py = qy0 + 8 * (k >> 1);
    const bool in = px < c.W && py < c.H;
    const size_t pix = in ? (size_t)py * c.W + px : 0;
    p[k].T = 1.0f;
    p[k].last = in ? n_contrib[pix] : 0u;
#pragma unroll
    for (int ch = 0; ch < FEAT_G; ch++) g[k][ch] = in && c0 + ch < C ? dL_dout[(size_t)(c0 + ch) * HW + pix] : 0.0f;
  }
  const float pfx0 = (float)qx0, pfy0 = (float)qy0;

  const uint32_t e_last = n_eff - 1;
  const uint32_t* const plist = point_list + t.range.x;
  auto pos = [&](uint32_t e) { return min(e, e_last); };
  uint32_t slot_c = plist[pos((uint32_t)lane)];
  uint32_t G1 = point_gid[slot_c];
  float4 pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
  uint32_t S1 = plist[pos((uint32_t)lane + 64u)];
  G1 = point_gid[S1];
  uint32_t S2 = plist[pos((uint32_t)lane + 128u)];

  // the previous batch's records, held by the lanes that staged its entries
  float4 pend0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pend1 = pend0;
  uint32_t pend_slot = 0, pend_n = 0;
  auto store_records = [&]() {
    if ((uint32_t)lane < pend_n) {
      rec[2 * (size_t)pend_slot] = pend0;
      rec[2 * (size_t)pend_slot + 1] = pend1;
    }
  };
  for (uint32_t base = 0; base < n_eff; base += 64) {
    const uint32_t cnt = min(64u, n_eff - base);
    const bool mine = (uint32_t)lane < cnt;
    const uint32_t slot = slot_c;
    uint32_t qmask = 0;
    if (mine) {
      s_xy[lane] = make_float2(pa.x, pa.y);
      s_co[lane] = fall_coefs_m<EXACT>(pa.z, pa.w, pb.x, pb.y);
      qmask = quadrant_mask(pa.x, pa.y, pa.z, pa.w, pb.x, pd.z, tx, ty);
    }
    slot_c = S1;
    pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
    S1 = S2;
    G1 = point_gid[S2];
    S2 = plist[pos(base + 192u + (uint32_t)lane)];
    // the previous batch's records, behind this batch's loads (loads and stores share one counter)
    if (base > 0) store_records();
    uint64_t M[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint64_t mk = __ballot((qmask >> k) & 1u);
      const uint32_t jn = t.qlast[k] > base ? t.qlast[k] - base : 0u;
      if (jn < 64u) mk &= (1ull << jn) - 1ull;
      M[k] = mk;
    }
    __builtin_amdgcn_wave_barrier();
    uint64_t m = (M[0] | M[1]) | (M[2] | M[3]);
    uint64_t wrote = 0;
#pragma unroll 1
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const float2 xy = s_xy[j];
      const float4 co = s_co[j];
      const uint32_t e = base + j;
      float s[FEAT_G];
#pragma unroll
      for (int ch = 0; ch < FEAT_G; ch++) s[ch] = 0.0f;
      uint64_t hit = 0;  // lanes with a pixel where the entry is composited
#pragma unroll
      for (int k = 0; k < 4; k++)
        if ((M[k] >> j) & 1ull) {
          bool con;
          const float a =
              feat_alpha<EXACT>(p[k], pfx0 + (float)(8 * (k & 1)), pfy0 + (float)(8 * (k >> 1)), xy, co, e, con);
          const float w = a * p[k].T;
          feat_step_T<EXACT>(p[k], a);
          // the lane's slot terms in slot order, each one product
#pragma unroll
          for (int ch = 0; ch < FEAT_G; ch++) s[ch] = s[ch] + g[k][ch] * w;
          hit |= __builtin_amdgcn_ballot_w64(con);
        }
      if (hit != 0) {
        wrote |= 1ull << j;
        wave_sumN_to_lane63<FEAT_G>(s);  // the steps of wave_sum_to_lane63, the channels interleaved
        if (lane == 63) {
          s_rec[j][0] = make_float4(s[0], s[1], s[2], s[3]);
          s_rec[j][1] = make_float4(s[4], s[5], s[6], s[7]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    // flush: lane t takes its entry's record (zeros for an entry no pixel composited); stored by the
    // next batch (or after the loop)
    pend0 = pend1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (mine && ((wrote >> lane) & 1ull)) {
      pend0 = s_rec[lane][0];
      pend1 = s_rec[lane][1];
    }
    pend_slot = slot;
    pend_n = cnt;
    __builtin_amdgcn_wave_barrier();  // the next batch overwrites the staged entries
  }
  store_records();
}

// ------------------------------------------------------------------------------------------
// per-Gaussian reduce: k_contrib_sum's sweep (a wave takes 64 consecutive depth ranks and sweeps
// their records 64 at a time, a segmented inclusive wave scan combines the records of one owner
// in slot order and the segment's last lane folds the partial into the owner's LDS accumulators)
// with FEAT_G fp64 sums.  Thread i of the grid also owns row i as a Gaussian index: rows without
// instances are zero-filled there (the group's columns), so a call that does not accumulate
// writes all P rows.
// ------------------------------------------------------------------------------------------
constexpr int FSUM_WAVES = 4;
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t feat_dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
// one step of the segmented scan (owners are carried +1 so a lane without a source (0) never matches
// a lane that holds a record; lanes without a record hold zeros)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void feat_scan_step(double (&s)[FEAT_G], uint32_t own1) {
  const bool same = feat_dpp_u<CTRL, ROW_MASK>(own1) == own1;
#pragma unroll
  for (int ch = 0; ch < FEAT_G; ch++) {
    const uint32_t lo = feat_dpp_u<CTRL, ROW_MASK>((uint32_t)__double2loint(s[ch]));
    const uint32_t hi = feat_dpp_u<CTRL, ROW_MASK>((uint32_t)__double2hiint(s[ch]));
    const double t = __hiloint2double((int)hi, (int)lo);
    s[ch] = same ? s[ch] + t : s[ch];
  }
}

__global__ __launch_bounds__(64 * FSUM_WAVES) void k_feature_sum(const uint32_t* __restrict__ counters,
                                                                 const uint32_t* __restrict__ offsets,
                                                                 const uint32_t* __restrict__ sorted_gid,
                                                                 const uint32_t* __restrict__ tiles,
                                                                 const uint32_t* __restrict__ slot_tile,
                                                                 const uint32_t* __restrict__ tile_cut,
                                                                 const uint32_t* __restrict__ cut_max,
                                                                 const float4* __restrict__ rec, uint32_t P, int C,
                                                                 int c0, float* __restrict__ dfeat, int accumulate) {
  __shared__ double s_sum[FSUM_WAVES][64][FEAT_G];
  __shared__ unsigned long long s_mark[FSUM_WAVES];
  const uint32_t V = counters[CNT_V], I = counters[CNT_I];
  const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t r0 = (blockIdx.x * FSUM_WAVES + wid) * 64;
  const int nc = min(FEAT_G, C - c0);  // the group's columns of a row
  // the forward's instance list is invalid (reported by the host): no valid records, zero gradients
  const bool invalid = (counters[CNT_ERR] & ERR_INVALID) != 0;
  if (!accumulate && r0 + lane < P && (invalid || tiles[r0 + lane] == 0)) {
    float* row = dfeat + (size_t)(r0 + lane) * (size_t)C + c0;
    for (int ch = 0; ch < nc; ch++) row[ch] = 0.0f;
  }
  if (invalid || r0 >= V) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t nr = min(64u, V - r0);
  const uint32_t my_off = lane < nr ? offsets[r0 + lane] : 0xFFFFFFFFu;
  const uint32_t S0 = (uint32_t)__shfl((int)my_off, 0, 64);
  // the wave's records end at its last owner's end or at the largest tile cut, whichever is first
  const uint32_t S1 = min((r0 + 64 < V) ? offsets[r0 + 64] : I, *cut_max);
#pragma unroll
  for (int ch = 0; ch < FEAT_G; ch++) s_sum[wid][lane][ch] = 0.0;
  const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  uint32_t jbase = 0xFFFFFFFFu;  // (number of owners starting before `base`) - 1
  // records of the next chunk are loaded one chunk ahead; records past their tile's cut were never
  // written: zeros (no load)
  const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 vn0 = z4, vn1 = z4;
  unsigned long long hn;
  {
    const uint32_t kk = S0 + lane;
    const bool h = kk < S1 && kk < tile_cut[slot_tile[kk]];
    if (h) vn0 = rec[2 * (size_t)kk], vn1 = rec[2 * (size_t)kk + 1];
    hn = __ballot(h);
  }
  for (uint32_t base = S0; base < S1; base += 64) {
    const float4 v0 = vn0, v1 = vn1;
    const unsigned long long hc = hn;
    if (base + 64 < S1) {
      const uint32_t kn = base + 64 + lane;
      vn0 = vn1 = z4;
      const bool h = kn < S1 && kn < tile_cut[slot_tile[kn]];
      if (h) vn0 = rec[2 * (size_t)kn], vn1 = rec[2 * (size_t)kn + 1];
      hn = __ballot(h);
    }
    if (hc == 0) {
      // no record in the chunk: only count the owners that start in it
      jbase += (uint32_t)__popcll(__ballot(my_off >= base && my_off < base + 64));
      continue;
    }
    // slots of the chunk that start an owner -> bit mask -> owner of my slot by popcount
    if (lane == 0) s_mark[wid] = 0ull;
    __builtin_amdgcn_wave_barrier();
    if (my_off >= base && my_off < base + 64) atomicOr(&s_mark[wid], 1ull << (my_off - base));
    __builtin_amdgcn_wave_barrier();
    const unsigned long long B = s_mark[wid];
    const uint32_t own = jbase + (uint32_t)__popcll(B & le);
    jbase += (uint32_t)__popcll(B);
    const bool valid = base + lane < S1;
    const float v[FEAT_G] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    double s[FEAT_G];
#pragma unroll
    for (int ch = 0; ch < FEAT_G; ch++) s[ch] = valid ? (double)v[ch] : 0.0;
    const uint32_t own1 = valid ? own + 1 : 0;
    feat_scan_step<0x111, 0xF>(s, own1);  // row_shr:1
    feat_scan_step<0x112, 0xF>(s, own1);  // row_shr:2
    feat_scan_step<0x114, 0xF>(s, own1);  // row_shr:4
    feat_scan_step<0x118, 0xF>(s, own1);  // row_shr:8
    feat_scan_step<0x142, 0xA>(s, own1);  // row_bcast:15 -> rows 1, 3
    feat_scan_step<0x143, 0xC>(s, own1);  // row_bcast:31 -> rows 2, 3
    const uint32_t next1 = (uint32_t)__shfl_down((int)own1, 1, 64);
    if (valid && (lane == 63 || next1 != own1)) {  // one lane per owner, chunks in order
#pragma unroll
      for (int ch = 0; ch < FEAT_G; ch++) s_sum[wid][own][ch] = s_sum[wid][own][ch] + s[ch];
    }
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < nr) {
    float* row = dfeat + (size_t)sorted_gid[r0 + lane] * (size_t)C + c0;
    for (int ch = 0; ch < nc; ch++) {
      const float s = (float)s_sum[wid][lane][ch];
      row[ch] = accumulate ? row[ch] + s : s;
    }
  }
}

void feature_forward(int P, int C, const CameraArgs& c, const GeomPtrs& geo, const BinPtrs& bin, const ImgPtrs& img,
                     const float* features, float* out, hipStream_t st) {
  (void)P;
  // the launch order of the view (and its record cuts): the backward's own kernel, which writes the
  // same words whenever it runs
  bwd_tile_order(c, bin, img, st);
  const dim3 grid((uint32_t)(c.gx * c.gy), (uint32_t)((C + FEAT_G - 1) / FEAT_G));
  with_flag(exact_exp(), [&](auto EXACT) {
    GS_LAUNCH("feature_fwd", k_feature_fwd<decltype(EXACT)::value>, grid, dim3(64), 0, st, c, img.ranges,
              bin.point_list, bin.presort_gid, geo.splat, img.n_contrib, img.tile_max, img.tile_order,
              &geo.counters[CNT_ERR], features, C, out);
  });
}

void feature_backward(int P, int C, const CameraArgs& c, const GeomPtrs& geo, const BinPtrs& bin, const ImgPtrs& img,
                      const float* dL_dout, void* scratch, float* dL_dfeatures, bool accumulate, hipStream_t st) {
  float4* rec = (float4*)scratch;
  bwd_tile_order(c, bin, img, st);
  const uint32_t slots = (uint32_t)(c.gx * c.gy);
  const dim3 sgrid((P + 64 * FSUM_WAVES - 1) / (64 * FSUM_WAVES)), sblock(64 * FSUM_WAVES);
  // the groups reuse the records in stream order
  for (int c0 = 0; c0 < C; c0 += FEAT_G) {
    with_flag(exact_exp(), [&](auto EXACT) {
      GS_LAUNCH("feature_bwd_walk", k_feature_bwd_walk<decltype(EXACT)::value>, dim3(slots), dim3(64), 0, st, c,
                img.ranges, bin.point_list, bin.presort_gid, geo.splat, img.n_contrib, img.tile_max, img.tile_order,
                dL_dout, C, c0, rec);
    });
    GS_LAUNCH("feature_sum", k_feature_sum, sgrid, sblock, 0, st, geo.counters, geo.offsets, geo.sorted_gid, geo.tiles,
              bin.slot_tile, img.tile_cut, img.cut_max, rec, (uint32_t)P, C, c0, dL_dfeatures, accumulate ? 1 : 0);
  }
}

}  // namespace gs
