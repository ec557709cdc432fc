// gs_contrib.hip -- per-Gaussian contribution statistics of one rendered view (gfx950).
//
// For Gaussian i and pixel p let "composited" mean what the colour forward decided (entry index <
// n_contrib[p], alpha = min(0.99, o G) >= 1/255, exact mode: power <= 0; the entry that stops a
// pixel is not composited) and w_i(p) = alpha_i(p) T_i(p), one fp32 product of the forward's own
// floats.  With an optional per-pixel weight map m >= 0 (none: 1) the view's statistics are
//   wsum[i]  = sum_p m_p w_i(p)        wmax[i] = max_p m_p w_i(p)
//   count[i] = #{p : i composited at p and m_p != 0}
// The kernel pair is the small sibling of the tile-wave backward and its record sums
// (gs_backward.hip):
//   k_contrib_walk  one wave per tile, four pixel slots per lane, 64-entry batches staged in LDS
//                   with the per-quadrant cull, walked FRONT TO BACK from T = 1 (the forward's own
//                   recurrence -- no final_T, no reciprocal); per walked entry one sum, one max and
//                   one popcount over the wave, and one 12-B record (wsum, wmax, count) per
//                   (tile, Gaussian) instance stored at the instance's slot (36 B in the backward).
//   k_contrib_sum   per Gaussian over its contiguous slot range, cut by tile_cut: the sum in fp64
//                   in slot order and rounded once, the max, the integer count; scattered to the
//                   Gaussian's row (written, or combined in place when accumulating).
// No float atomics on global memory and a fixed order everywhere: bitwise reproducible.
#include "gs_internal.h"

namespace gs {

struct __attribute__((aligned(4))) ContribRec {
  float wsum, wmax;
  uint32_t count;
};

struct ContribSlot {
  float T, m;     // transmittance in front of the next entry; the pixel's weight (0 outside the image)
  uint32_t last;  // n_contrib of the pixel (0 outside the image)
};

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}

// one slot's evaluation for one entry: the forward's decision and recurrence of the numerics mode;
// s / mx take the lane's slots in slot order.  Returns the lanes where the entry is composited.
// mx is the running maximum as the float's bits: the terms are >= +0, where the unsigned order of
// the bits is the order of the floats, and an integer max needs no canonicalising v_max_f32 x, x
// in front of it and folds its DPP move (20 VALU fewer per reduced entry in the ISA).
template <bool EXACT>
__device__ __forceinline__ uint64_t contrib_slot(ContribSlot& q, float pfx, float pfy, const float2 xy, const float4 co,
                                                 uint32_t e, float& s, uint32_t& mx) {
  const float dx = xy.x - pfx, dy = xy.y - pfy;
  const float pw = falloff_log2_m<EXACT>(co, dx, dy);  // log2(e) * power (fast: + log2 o)
  const float oG = opac_gauss<EXACT>(co, pw);
  // the conditions of bwd_slot (and of the forward's walk)
  const bool c_walk = e < q.last, c_alpha = oG >= 1.0f / 255.0f, c_pw = !EXACT || pw <= 0.0f;
  const bool con = c_walk && c_pw && c_alpha;
  // a pixel where the entry is not composited runs as an alpha 0 entry: T passes through bit for bit
  const float a = con ? fminf(0.99f, oG) : 0.0f;
  const float w = a * q.T;
  if constexpr (EXACT)
    q.T = q.T * (1.0f - a);
  else
    q.T = __builtin_fmaf(-a, q.T, q.T);
  const float mw = q.m * w;
  s = s + mw;
  mx = max(mx, __float_as_uint(mw));
  uint64_t m = __builtin_amdgcn_ballot_w64(c_walk) & __builtin_amdgcn_ballot_w64(c_alpha);
  if constexpr (EXACT) m &= __builtin_amdgcn_ballot_w64(c_pw);
  return m;
}

// 64-lane sum of s and max of m (bits of floats >= +0: a lane without a source reads 0), both in
// lane 63; the steps of wave_sum_to_lane63, interleaved
__device__ __forceinline__ void wave_sum_max_to_lane63(float& s, uint32_t& m) {
#define GS_STEP(...)                           \
  {                                            \
    const float ts = dpp_f<__VA_ARGS__>(s);    \
    const uint32_t tm = dpp_u<__VA_ARGS__>(m); \
    s = s + ts;                                \
    m = max(m, tm);                            \
  }
  GS_STEP(0xB1)        // quad_perm [1,0,3,2]
  GS_STEP(0x4E)        // quad_perm [2,3,0,1]
  GS_STEP(0x141)       // row_half_mirror
  GS_STEP(0x140)       // row_mirror
  GS_STEP(0x142, 0xA)  // row_bcast:15 -> rows 1, 3
  GS_STEP(0x143, 0xC)  // row_bcast:31 -> rows 2, 3
#undef GS_STEP
}

template <bool EXACT>
__global__ __launch_bounds__(64) void k_contrib_walk(CameraArgs c, const uint2* __restrict__ ranges,
                                                     const uint32_t* __restrict__ point_list,
                                                     const uint32_t* __restrict__ point_gid,
                                                     const float4* __restrict__ splat,
                                                     const uint32_t* __restrict__ n_contrib,
                                                     const uint32_t* __restrict__ tile_max,
                                                     const uint32_t* __restrict__ tile_order,
                                                     const float* __restrict__ weights,
                                                     ContribRec* __restrict__ rec) {
  __shared__ float2 s_xy[64];
  __shared__ float4 s_co[64];   // falloff coefficients + opacity (fall_coefs)
  __shared__ float4 s_rec[64];  // (wsum, wmax, bits(count), -) of the batch's entries
  const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_order ? tile_order[blockIdx.x] : blockIdx.x);
  if (tile == ~0u) return;  // a hole of the XCD-group launch order
  const int tx = (int)(tile % (uint32_t)c.gx), ty = (int)(tile / (uint32_t)c.gx);
  const int lane = threadIdx.x;
  const uint2 range = ranges[tile];
  const uint32_t n = range.y - range.x;
  // per-quadrant largest n_contrib (the forward's quadrant waves): slot k's walk ends there
  const uint4 qm = reinterpret_cast<const uint4*>(tile_max)[tile];
  const uint32_t qlast[4] = {min(qm.x, n), min(qm.y, n), min(qm.z, n), min(qm.w, n)};
  const uint32_t n_eff = max(max(qlast[0], qlast[1]), max(qlast[2], qlast[3]));
  if (n_eff == 0) return;  // no instance walked: no records (k_contrib_sum reads none below a cut of 0)

  const int qx0 = tx * GS_TILE + (lane & 7), qy0 = ty * GS_TILE + (lane >> 3);
  ContribSlot p[4];
  uint64_t mnz[4];  // lanes whose pixel of slot k has a non-zero weight
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int px = qx0 + 8 * (k & 1), py = qy0 + 8 * (k >> 1);
    const bool in = px < c.W && py < c.H;
    const size_t pix = in ? (size_t)py * c.W + px : 0;
    p[k].T = 1.0f;
    p[k].last = in ? n_contrib[pix] : 0u;
    // (+ 0: a weight of -0 counts as 0, and the terms keep the sign bit clear)
    p[k].m = in ? (weights ? weights[pix] + 0.0f : 1.0f) : 0.0f;
    mnz[k] = __builtin_amdgcn_ballot_w64(p[k].m != 0.0f);
  }
  const float pfx0 = (float)qx0, pfy0 = (float)qy0;

  // staging pipeline (one entry per lane), as in k_render_bwd_tw but front to back: while batch k is
  // walked, the splat records of batch k + 1, the ids of batch k + 2 and the slots of batch k + 3
  // are in flight.  Batch k's entry of lane t is entry 64 k + t of the tile's list; the loads are
  // unconditional, with entries past the walk's end clamped to its last one (a valid entry: the
  // lane stages nothing then).
  const uint32_t e_last = n_eff - 1;
  const uint32_t* const plist = point_list + range.x;
  auto pos = [&](uint32_t e) { return min(e, e_last); };
  uint32_t slot_c = plist[pos((uint32_t)lane)];
  uint32_t G1 = point_gid[slot_c];
  float4 pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
  uint32_t S1 = plist[pos((uint32_t)lane + 64u)];
  G1 = point_gid[S1];
  uint32_t S2 = plist[pos((uint32_t)lane + 128u)];

  // the previous batch's records, held by the lanes that staged its entries
  ContribRec pend = {0.0f, 0.0f, 0u};
  uint32_t pend_slot = 0, pend_n = 0;
  auto store_records = [&]() {
    if ((uint32_t)lane < pend_n) rec[pend_slot] = pend;
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
    // issue the next batch's splat loads, the ids after it and the slots after those
    slot_c = S1;
    pa = splat[3 * G1], pb = splat[3 * G1 + 1], pd = splat[3 * G1 + 2];
    S1 = S2;
    G1 = point_gid[S2];
    S2 = plist[pos(base + 192u + (uint32_t)lane)];
    // the previous batch's records, behind this batch's loads (loads and stores share one counter)
    if (base > 0) store_records();
    // per-slot entry sets: entry j of the batch reaches quadrant k iff base + j < qlast[k]
    uint64_t M[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint64_t mk = __ballot((qmask >> k) & 1u);
      const uint32_t jn = qlast[k] > base ? qlast[k] - base : 0u;
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
      float s = 0.0f;
      uint32_t mx = 0u;
      uint32_t hits = 0;  // pixels where the entry is composited under a non-zero weight
#pragma unroll
      for (int k = 0; k < 4; k++)
        if ((M[k] >> j) & 1ull)
          hits += (uint32_t)__popcll(mnz[k] & contrib_slot<EXACT>(p[k], pfx0 + (float)(8 * (k & 1)),
                                                                  pfy0 + (float)(8 * (k >> 1)), xy, co, e, s, mx));
      if (hits != 0) {
        wrote |= 1ull << j;
        wave_sum_max_to_lane63(s, mx);
        if (lane == 63) s_rec[j] = make_float4(s, __uint_as_float(mx), __uint_as_float(hits), 0.0f);
      }
    }
    __builtin_amdgcn_wave_barrier();
    // flush: lane t takes its entry's record (zeros for an entry no weighted pixel took); stored by
    // the next batch (or after the loop)
    pend = ContribRec{0.0f, 0.0f, 0u};
    if (mine && ((wrote >> lane) & 1ull)) {
      const float4 r = s_rec[lane];
      pend = ContribRec{r.x, r.y, __float_as_uint(r.z)};
    }
    pend_slot = slot;
    pend_n = cnt;
    __builtin_amdgcn_wave_barrier();  // the next batch overwrites the staged entries
  }
  store_records();
}

// ------------------------------------------------------------------------------------------
// per-Gaussian reduce, in the style of k_sum_records: a wave takes 64 consecutive depth ranks and
// sweeps their records 64 at a time; a segmented inclusive wave scan (fp64 sum, max, integer sum)
// combines the records of one owner in slot order and the segment's last lane folds the partial
// into the owner's LDS accumulators (one lane per owner and chunk, chunks in order: no atomics).
// Thread i of the grid also owns row i as a Gaussian index: rows without instances are zero-filled
// there, so a call that does not accumulate writes all P rows.
// ------------------------------------------------------------------------------------------
constexpr int CSUM_WAVES = 4;
// one step of the segmented scan (owners are carried +1 so a lane without a source (0) never matches
// a lane that holds a record; lanes without a record hold zeros)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void contrib_scan_step(double& s, float& mx, uint32_t& n, uint32_t own1) {
  const bool same = dpp_u<CTRL, ROW_MASK>(own1) == own1;
  const uint32_t lo = dpp_u<CTRL, ROW_MASK>((uint32_t)__double2loint(s));
  const uint32_t hi = dpp_u<CTRL, ROW_MASK>((uint32_t)__double2hiint(s));
  const float m2 = __uint_as_float(dpp_u<CTRL, ROW_MASK>(__float_as_uint(mx)));
  const uint32_t n2 = dpp_u<CTRL, ROW_MASK>(n);
  const double t = __hiloint2double((int)hi, (int)lo);
  s = same ? s + t : s;
  mx = same ? fmaxf(mx, m2) : mx;
  n = same ? n + n2 : n;
}

__global__ __launch_bounds__(64 * CSUM_WAVES) void k_contrib_sum(const uint32_t* __restrict__ counters,
                                                                 const uint32_t* __restrict__ offsets,
                                                                 const uint32_t* __restrict__ sorted_gid,
                                                                 const uint32_t* __restrict__ tiles,
                                                                 const uint32_t* __restrict__ slot_tile,
                                                                 const uint32_t* __restrict__ tile_cut,
                                                                 const uint32_t* __restrict__ cut_max,
                                                                 const ContribRec* __restrict__ rec, uint32_t P,
                                                                 float* __restrict__ wsum, float* __restrict__ wmax,
                                                                 int* __restrict__ count, int accumulate) {
  __shared__ double s_sum[CSUM_WAVES][64];
  __shared__ float s_max[CSUM_WAVES][64];
  __shared__ uint32_t s_cnt[CSUM_WAVES][64];
  __shared__ unsigned long long s_mark[CSUM_WAVES];
  const uint32_t V = counters[CNT_V], I = counters[CNT_I];
  const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t r0 = (blockIdx.x * CSUM_WAVES + wid) * 64;
  // the forward's instance list is invalid (reported by the host): no valid records, zero statistics
  const bool invalid = (counters[CNT_ERR] & ERR_INVALID) != 0;
  if (!accumulate && r0 + lane < P && (invalid || tiles[r0 + lane] == 0)) {
    if (wsum) wsum[r0 + lane] = 0.0f;
    if (wmax) wmax[r0 + lane] = 0.0f;
    if (count) count[r0 + lane] = 0;
  }
  if (invalid || r0 >= V) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t nr = min(64u, V - r0);
  const uint32_t my_off = lane < nr ? offsets[r0 + lane] : 0xFFFFFFFFu;
  const uint32_t S0 = (uint32_t)__shfl((int)my_off, 0, 64);
  // the wave's records end at its last owner's end or at the largest tile cut, whichever is first
  const uint32_t S1 = min((r0 + 64 < V) ? offsets[r0 + 64] : I, *cut_max);
  s_sum[wid][lane] = 0.0;
  s_max[wid][lane] = 0.0f;
  s_cnt[wid][lane] = 0u;
  const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  uint32_t jbase = 0xFFFFFFFFu;  // (number of owners starting before `base`) - 1
  // records of the next chunk are loaded one chunk ahead; records past their tile's cut were never
  // written: zeros (no load)
  ContribRec vn = {0.0f, 0.0f, 0u};
  unsigned long long hn;
  {
    const uint32_t kk = S0 + lane;
    const bool h = kk < S1 && kk < tile_cut[slot_tile[kk]];
    if (h) vn = rec[kk];
    hn = __ballot(h);
  }
  for (uint32_t base = S0; base < S1; base += 64) {
    const ContribRec v = vn;
    const unsigned long long hc = hn;
    if (base + 64 < S1) {
      const uint32_t kn = base + 64 + lane;
      vn = ContribRec{0.0f, 0.0f, 0u};
      const bool h = kn < S1 && kn < tile_cut[slot_tile[kn]];
      if (h) vn = rec[kn];
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
    double s = valid ? (double)v.wsum : 0.0;
    float mx = valid ? v.wmax : 0.0f;
    uint32_t nn = valid ? v.count : 0u;
    const uint32_t own1 = valid ? own + 1 : 0;
    contrib_scan_step<0x111, 0xF>(s, mx, nn, own1);  // row_shr:1
    contrib_scan_step<0x112, 0xF>(s, mx, nn, own1);  // row_shr:2
    contrib_scan_step<0x114, 0xF>(s, mx, nn, own1);  // row_shr:4
    contrib_scan_step<0x118, 0xF>(s, mx, nn, own1);  // row_shr:8
    contrib_scan_step<0x142, 0xA>(s, mx, nn, own1);  // row_bcast:15 -> rows 1, 3
    contrib_scan_step<0x143, 0xC>(s, mx, nn, own1);  // row_bcast:31 -> rows 2, 3
    const uint32_t next1 = (uint32_t)__shfl_down((int)own1, 1, 64);
    if (valid && (lane == 63 || next1 != own1)) {  // one lane per owner, chunks in order
      s_sum[wid][own] = s_sum[wid][own] + s;
      s_max[wid][own] = fmaxf(s_max[wid][own], mx);
      s_cnt[wid][own] = s_cnt[wid][own] + nn;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < nr) {
    const size_t gid = sorted_gid[r0 + lane];
    const float s = (float)s_sum[wid][lane], mx = s_max[wid][lane];
    const int nn = (int)s_cnt[wid][lane];
    if (accumulate) {
      if (wsum) wsum[gid] = wsum[gid] + s;
      if (wmax) wmax[gid] = fmaxf(wmax[gid], mx);
      if (count) count[gid] = count[gid] + nn;
    } else {
      if (wsum) wsum[gid] = s;
      if (wmax) wmax[gid] = mx;
      if (count) count[gid] = nn;
    }
  }
}

void contrib_stats(int P, const CameraArgs& c, const GeomPtrs& geo, const BinPtrs& bin, const ImgPtrs& img,
                   const float* weights, void* scratch, float* wsum, float* wmax, int* count, bool accumulate,
                   hipStream_t st) {
  ContribRec* rec = (ContribRec*)scratch;
  // the launch order and the record cuts (tile_cut, cut_max) of the view: the backward's own
  // kernel, which writes the same words whenever it runs
  bwd_tile_order(c, bin, img, st);
  const uint32_t slots = (uint32_t)(c.gx * c.gy);
  with_flag(exact_exp(), [&](auto EXACT) {
    GS_LAUNCH("contrib_walk", k_contrib_walk<decltype(EXACT)::value>, dim3(slots), dim3(64), 0, st, c, img.ranges,
              bin.point_list, bin.presort_gid, geo.splat, img.n_contrib, img.tile_max, img.tile_order, weights, rec);
  });
  const dim3 grid((P + 64 * CSUM_WAVES - 1) / (64 * CSUM_WAVES)), block(64 * CSUM_WAVES);
  GS_LAUNCH("contrib_sum", k_contrib_sum, grid, block, 0, st, geo.counters, geo.offsets, geo.sorted_gid, geo.tiles,
            bin.slot_tile, img.tile_cut, img.cut_max, rec, (uint32_t)P, wsum, wmax, count, accumulate ? 1 : 0);
}

}  // namespace gs
