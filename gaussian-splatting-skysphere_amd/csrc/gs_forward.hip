// gs_forward.hip -- forward pass of the MI355X Gaussian rasterizer (gfx950).
//
// Restates the un-vendored upstream forward (graphdeco-inria/diff-gaussian-rasterization,
// /root/reference/.gitmodules:4-6; spec SURVEY.md §8a a4-a6) as:
//   k_preprocess   one lane per Gaussian: cull, project, cov3D -> EWA cov2D -> conic, radius,
//                  tile rectangle, SH -> RGB; writes the 48-B splat record used by render.
//   fwd_order      stable 32-bit depth radix sort of the Gaussians with instances (the first
//                  pass drops the others: compaction), exclusive scan of their tile counts in
//                  depth order.
//   k_duplicate    one lane per depth-ranked Gaussian writes its (tile, slot) instances; slots of
//                  a Gaussian are contiguous and in depth order.
//   tile sort      stable radix sort of the instances by tile id only: because the input is
//                  already depth-ordered (ties by Gaussian index) this equals upstream's sort by
//                  the 64-bit key (tile << 32 | depth bits) with a ~3x smaller sort.
//   k_ranges       per-tile [start, end) of the sorted list.  (Two-pass tile sorts of large enough
//                  buffers run packed -- one word per instance, no sorted keys -- and take their
//                  ranges from the second pass's histogram: tile_sort_packed_views.)
//   k_render_fwd   one 256-lane workgroup (4 wave64) per 16x16 tile; Gaussians staged through LDS
//                  256 at a time; front-to-back compositing with the block-wide early exit.
#include "gs_internal.h"

namespace gs {

// ------------------------------------------------------------------------------------------
// preprocess
// ------------------------------------------------------------------------------------------

// SH -> RGB for one Gaussian, channel-major evaluation order identical to oracle/gs_oracle.c
// sh_eval_one (reference: /root/reference/utils/sh_utils.py:57-100, +0.5 and clamp_min(0) as
// /root/reference/gaussian_renderer/__init__.py:77-78).
// split: split rows (sh = the Gaussian's features_dc row, rest = its features_rest row),
// read as 12-B pieces; the evaluation is the same.
// The Gaussian's 3 (DEG + 1)^2 coefficients s[3 k + c] from its global row(s); split: a uniform flag.
template <int DEG>
__device__ __forceinline__ void sh_row_load(const float* __restrict__ sh, const float* __restrict__ rest, bool split,
                                            int M, float* s) {
  constexpr int K = (DEG + 1) * (DEG + 1);
  if (split) {
    const F3 d = *reinterpret_cast<const F3*>(sh);
    s[0] = d.a, s[1] = d.b, s[2] = d.c;
    const F3* r3 = reinterpret_cast<const F3*>(rest);
#pragma unroll
    for (int j = 0; j < K - 1; j++) {
      const F3 t = r3[j];
      s[3 + 3 * j] = t.a, s[4 + 3 * j] = t.b, s[5 + 3 * j] = t.c;
    }
  } else if (((M * 3) & 3) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(sh);
#pragma unroll
    for (int v = 0; v < (K * 3 + 3) / 4; v++) {
      float4 q = s4[v];
      if (4 * v + 0 < K * 3) s[4 * v + 0] = q.x;
      if (4 * v + 1 < K * 3) s[4 * v + 1] = q.y;
      if (4 * v + 2 < K * 3) s[4 * v + 2] = q.z;
      if (4 * v + 3 < K * 3) s[4 * v + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < K * 3; k++) s[k] = sh[k];
  }
}
// The same coefficients from the Gaussian's staged LDS row (stage_sh_rows): whole 16-B reads.
template <int DEG>
__device__ __forceinline__ void sh_row_load_lds(const float* row, float* s) {
  constexpr int KF = 3 * (DEG + 1) * (DEG + 1);
  static_assert(KF % 4 == 0, "staged rows are whole 16-B pieces");
#pragma unroll
  for (int q = 0; q < KF / 4; q++) {
    const float4 t = lds_ld16(row + 4 * q);
    s[4 * q + 0] = t.x, s[4 * q + 1] = t.y, s[4 * q + 2] = t.z, s[4 * q + 3] = t.w;
  }
}
template <int DEG>
__device__ __forceinline__ void sh_eval(const float* s, float x, float y, float z, float* rgb, uint32_t& clamped) {
  clamped = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
#define S(k) s[3 * (k) + c]
    float res = SH_C0 * S(0);
    if (DEG > 0) {
      res = res - (SH_C1 * y) * S(1) + (SH_C1 * z) * S(2) - (SH_C1 * x) * S(3);
      if (DEG > 1) {
        float xx = x * x, yy = y * y, zz = z * z;
        float xy = x * y, yz = y * z, xz = x * z;
        res = res + (SH_C20 * xy) * S(4) + (SH_C21 * yz) * S(5) + (SH_C22 * (2.0f * zz - xx - yy)) * S(6) +
              (SH_C23 * xz) * S(7) + (SH_C24 * (xx - yy)) * S(8);
        if (DEG > 2) {
          res = res + ((SH_C30 * y) * (3.0f * xx - yy)) * S(9) + ((SH_C31 * xy) * z) * S(10) +
                ((SH_C32 * y) * (4.0f * zz - xx - yy)) * S(11) +
                ((SH_C33 * z) * (2.0f * zz - 3.0f * xx - 3.0f * yy)) * S(12) +
                ((SH_C34 * x) * (4.0f * zz - xx - yy)) * S(13) + ((SH_C35 * z) * (xx - yy)) * S(14) +
                ((SH_C36 * x) * (xx - 3.0f * yy)) * S(15);
        }
      }
    }
#undef S
    res = res + 0.5f;
    if (res < 0.0f) clamped |= 1u << c;
    rgb[c] = res < 0.0f ? 0.0f : res;
  }
}

// Where preprocess_view finds the Gaussian's SH row:
//   ROW_GLOBAL  its global row g.shs[i], loaded by the lane where it is used
//   ROW_SPLIT   as ROW_GLOBAL, or features_dc + features_rest rows when g.shs_rest is set (a uniform
//               branch: with both row loaders in the kernel the scheduler keeps the split loads where
//               they are used, 91 VGPRs; a split-only instantiation hoists them, 130 VGPRs, 75 -> 97
//               us at C3)
//   ROW_LDS     the workgroup's rows staged in LDS (stage_sh_rows), read with whole 16-B LDS loads
//   ROW_REGS    loaded once by preprocess_shared and held in registers
enum RowSrc { ROW_GLOBAL = 0, ROW_SPLIT = 1, ROW_LDS = 2, ROW_REGS = 3 };

// floats of an SH row of degree DEG (3 for DEG = -1: the precomputed colour)
constexpr int sh_row_floats(int deg) { return deg < 0 ? 3 : 3 * (deg + 1) * (deg + 1); }

// The camera-independent half of one Gaussian's preprocess: mean, 3D covariance, opacity and its
// culling limit, and the colour source: the precomputed colour (DEG = -1), the coefficients
// (ROW_REGS) or the staged row's address (ROW_LDS); a global row is addressed by i (sh_row_of).
template <int DEG, int SRC>
struct PreShared {
  float px, py, pz;
  float cov3[6];
  float op, lim;
  const float* row;  // ROW_LDS: the staged SH row (global rows are addressed where they are loaded, sh_row_of)
  float s[(DEG < 0 || SRC == ROW_REGS) ? sh_row_floats(DEG) : 1];  // colour / coefficients held in registers
};

// SH -> RGB of Gaussian i from its global row(s), by the launch's layout.  A uniform branch around
// load + evaluation: with only the loads in the branches the compiler merges them into 48 one-dword
// loads through selected addresses (128 VGPRs in k_preprocess_split<3>).
template <int DEG, int SRC>
__device__ __forceinline__ void sh_rgb_of(int i, const GaussianArgs& g, float x, float y, float z, float* rgb,
                                          uint32_t& clamped) {
  float s[sh_row_floats(DEG)];
  if (SRC == ROW_SPLIT && g.shs_rest) {
    sh_row_load<DEG>(g.shs + (size_t)i * 3, g.shs_rest + (size_t)i * (g.M - 1) * 3, true, g.M, s);
    sh_eval<DEG>(s, x, y, z, rgb, clamped);
  } else {
    sh_row_load<DEG>(g.shs + (size_t)i * g.M * 3, nullptr, false, g.M, s);
    sh_eval<DEG>(s, x, y, z, rgb, clamped);
  }
}

// lds_row: the lane's staged row (ROW_LDS only).  HOIST = false (the single-view kernels): the opacity
// and its culling limit are left to preprocess_view, which takes them where they are stored, beside
// the SH row's loads -- loaded here, ahead of the near cull, the opacity's latency is exposed on its
// own (k_preprocess<3> at C3: 72 -> 91 us).
template <int DEG, int SRC, bool HOIST>
__device__ __forceinline__ PreShared<DEG, SRC> preprocess_shared(int i, const GaussianArgs& g, const float* lds_row) {
  PreShared<DEG, SRC> sh;
  sh.px = g.means3D[3 * i + 0], sh.py = g.means3D[3 * i + 1], sh.pz = g.means3D[3 * i + 2];
  if (g.cov3D) {
#pragma unroll
    for (int k = 0; k < 6; k++) sh.cov3[k] = g.cov3D[6 * i + k];
  } else {
    cov3d(g.scales[3 * i], g.scales[3 * i + 1], g.scales[3 * i + 2], g.scale_modifier, g.rotations[4 * i],
          g.rotations[4 * i + 1], g.rotations[4 * i + 2], g.rotations[4 * i + 3], sh.cov3);
  }
  // culling limit of the {alpha >= 1/255} ellipse (render-side work skipping only; never
  // changes a result, see ellipse_meets_rect): q(d) <= 2 ln(255 o), with safety margins
  sh.op = HOIST ? g.opacities[i] : 0.0f;
  sh.lim = HOIST ? cull_lim(sh.op) : 0.0f;
  sh.row = lds_row, sh.s[0] = 0.0f;
  if constexpr (DEG < 0) {
    sh.s[0] = g.colors[3 * i], sh.s[1] = g.colors[3 * i + 1], sh.s[2] = g.colors[3 * i + 2];
  } else if constexpr (SRC == ROW_REGS) {
    sh_row_load<DEG>(g.shs + (size_t)i * g.M * 3, nullptr, false, g.M, sh.s);
  }
  return sh;
}

// What one camera adds for Gaussian i: near cull, projection, EWA cov2D -> conic, radius and tile
// rectangle, SH -> RGB, the tile-exact row spans, and the stores of the view's outputs.  Returns the
// number of tiles the Gaussian touches (0 when culled; radii[i] and tiles[i] are then 0).
// AA (k_preprocess_aa): the antialiased opacity op s takes the opacity's place in the splat record
// and in the culling limit (aa_scale); everything else is the plain code.
template <int DEG, int SRC, bool HOIST, bool AA = false>
__device__ __forceinline__ uint32_t preprocess_view(int i, const PreShared<DEG, SRC>& sh, const GaussianArgs& g,
                                                    const CameraArgs& c,
                                                    int* __restrict__ radii, float4* __restrict__ splat,
                                                    float4* __restrict__ binrec, uint32_t& dbits,
                                                    uint32_t* __restrict__ tiles, uint8_t* __restrict__ clamped,
                                                    bool& culled_prefiltered) {
  const float px = sh.px, py = sh.py, pz = sh.pz;
  const float3v pv = xf43(c.view, px, py, pz);
  if (pv.z <= 0.2f) {
    culled_prefiltered = c.prefiltered != 0;  // upstream raises "Point is filtered although prefiltered is set"
    radii[i] = 0;
    tiles[i] = 0;
    return 0;
  }
  const float* P = c.proj;
  const float hx = P[0] * px + P[4] * py + P[8] * pz + P[12];
  const float hy = P[1] * px + P[5] * py + P[9] * pz + P[13];
  const float hw = xf44w(P, px, py, pz);
  const float pw = 1.0f / (hw + 0.0000001f);
  const float projx = hx * pw, projy = hy * pw;

  const Cov2D cv = cov2d(c.view, px, py, pz, sh.cov3, c.fx, c.fy, c.tanfovx, c.tanfovy);
  const float det = cv.a * cv.c - cv.b * cv.b;
  if (det == 0.0f) {
    radii[i] = 0;
    tiles[i] = 0;
    return 0;
  }
  const float det_inv = 1.f / det;
  const float cxx = cv.c * det_inv, cxy = -cv.b * det_inv, cyy = cv.a * det_inv;
  const float mid = 0.5f * (cv.a + cv.c);
  const float disc = fmaxf(0.1f, mid * mid - det);
  const float l1 = mid + sqrtf(disc), l2 = mid - sqrtf(disc);
  const int radius = (int)ceilf(3.f * sqrtf(fmaxf(l1, l2)));
  const float sx = ndc2pix(projx, c.W), sy = ndc2pix(projy, c.H);
  int x0, y0, x1, y1;
  get_rect(sx, sy, radius, c.gx, c.gy, x0, y0, x1, y1);
  const int area = (x1 - x0) * (y1 - y0);
  if (area == 0) {
    radii[i] = 0;
    tiles[i] = 0;
    return 0;
  }

  float rgb[3];
  uint32_t cl = 0;
  if constexpr (DEG < 0) {
    rgb[0] = sh.s[0], rgb[1] = sh.s[1], rgb[2] = sh.s[2];
  } else {
    float dx = px - c.campos[0], dy = py - c.campos[1], dz = pz - c.campos[2];
    float len = sqrtf(dx * dx + dy * dy + dz * dz);
    if constexpr (SRC == ROW_REGS) {
      sh_eval<DEG>(sh.s, dx / len, dy / len, dz / len, rgb, cl);
    } else if constexpr (SRC == ROW_LDS) {
      float s[sh_row_floats(DEG)];
      sh_row_load_lds<DEG>(sh.row, s);
      sh_eval<DEG>(s, dx / len, dy / len, dz / len, rgb, cl);
    } else {
      sh_rgb_of<DEG, SRC>(i, g, dx / len, dy / len, dz / len, rgb, cl);
    }
  }
  float op = HOIST ? sh.op : g.opacities[i];
  float lim;
  if constexpr (AA) {
    float r, D0;
    op = op * aa_scale(cv, det, r, D0);
    lim = cull_lim(op);
  } else {
    lim = HOIST ? sh.lim : cull_lim(op);
  }
  splat[3 * i + 0] = make_float4(sx, sy, cxx, cxy);
  splat[3 * i + 1] = make_float4(cyy, op, rgb[0], rgb[1]);
  splat[3 * i + 2] = make_float4(rgb[2], pv.z, lim, 0.0f);
  dbits = __float_as_uint(pv.z);
  radii[i] = radius;  // upstream visibility: the rectangle is non-empty
  // tile-exact instance count (may be 0 for a visible splat whose alpha never reaches 1/255)
  const SpanCtx sp = span_ctx(sx, sy, cxx, cxy, cyy, lim, x0, x1);
  uint32_t count = 0;
  for (int ty = y0; ty < y1; ty++) {
    int ta, tb;
    row_span(sp, ty, ta, tb);
    count += (uint32_t)(tb - ta);
  }
  binrec[2 * i + 0] = make_float4(sx, sy, cxx, cxy);
  binrec[2 * i + 1] = make_float4(cyy, lim, __uint_as_float((uint32_t)x0 | ((uint32_t)x1 << 16)),
                                  __uint_as_float((uint32_t)y0 | ((uint32_t)y1 << 16)));
  tiles[i] = count;
  clamped[i] = (uint8_t)cl;
  return count;
}


// The workgroup's tile total and count of Gaussians with instances (+ a prefiltered cull) -> its
// WgTotals slot; the first depth-sort histogram launch sums the slots (CounterFinalize).
__device__ __forceinline__ void workgroup_totals(uint32_t area, bool culled, WgTotals* wg, uint32_t b) {
  __shared__ uint32_t s_sum[4], s_vis[4];
  uint32_t vis = area ? 1u : 0u;
  const uint64_t cm = __ballot(culled);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    area += (uint32_t)__shfl_xor((int)area, d, 64);
    vis += (uint32_t)__shfl_xor((int)vis, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = area;
    s_vis[threadIdx.x >> 6] = vis | (cm ? 0x80000000u : 0u);
  }
  lds_barrier();
  if (threadIdx.x == 0) {
    const uint32_t tot = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const uint32_t v4 = s_vis[0] | s_vis[1] | s_vis[2] | s_vis[3];
    const uint32_t nv = (s_vis[0] & 0x7FFFFFFFu) + (s_vis[1] & 0x7FFFFFFFu) + (s_vis[2] & 0x7FFFFFFFu) +
                        (s_vis[3] & 0x7FFFFFFFu);
    store_wg_totals(wg, b, nv, tot, (v4 >> 31) != 0);
  }
}

// ROW_LDS: the rows of workgroup b's Gaussians, staged into the launch's dynamic LDS
// (sh_stage_bytes) with coalesced 16-B loads; returns the lane's row.  The loads are bounded by the
// rows that exist (a partial last workgroup), and every lane of the workgroup reaches the barrier.
template <int DEG>
__device__ __forceinline__ const float* stage_block_rows(const GaussianArgs& g, int b) {
  extern __shared__ __attribute__((aligned(16))) float s_sh_rows[];
  constexpr int KF = sh_row_floats(DEG);
  const int i0 = b * 256;
  stage_sh_rows<KF>(g.shs + (size_t)i0 * KF, min(256, g.P - i0), s_sh_rows);
  lds_barrier();
  return s_sh_rows + (int)threadIdx.x * sh_stage_stride(KF);
}

// The workgroup's tile total (num_rendered, read back by the host right after the first depth-sort
// histogram launch while the ordering kernels run) and its count of Gaussians with instances (V)
// go to its WgTotals slot (workgroup_totals).  depth_key[i] is the depth's bits for those and
// DEPTH_DROP for every other Gaussian: the first depth-sort pass drops them, which is the
// visibility compaction.
template <int DEG, int SRC, bool AA = false>
__device__ __forceinline__ void preprocess_block(const GaussianArgs& g, const CameraArgs& c, int* __restrict__ radii,
                                                 float4* __restrict__ splat, float4* __restrict__ binrec,
                                                 uint32_t* __restrict__ depth_key, uint32_t* __restrict__ tiles,
                                                 uint8_t* __restrict__ clamped, WgTotals* __restrict__ wg) {
  const int b = (int)blockIdx.x + g.blk0, i = b * 256 + (int)threadIdx.x;
  uint32_t area = 0, dbits = 0;
  bool culled = false;
  if (i < g.P) {
    const PreShared<DEG, SRC> sh = preprocess_shared<DEG, SRC, false>(i, g, nullptr);
    area = preprocess_view<DEG, SRC, false, AA>(i, sh, g, c, radii, splat, binrec, dbits, tiles, clamped, culled);
    depth_key[i] = area ? dbits : DEPTH_DROP;
  }
  workgroup_totals(area, culled, wg, (uint32_t)b);
}

template <int DEG>
__global__ __launch_bounds__(256) void k_preprocess(GaussianArgs g, CameraArgs c, int* __restrict__ radii,
                                                    float4* __restrict__ splat, float4* __restrict__ binrec,
                                                    uint32_t* __restrict__ depth_key,
                                                    uint32_t* __restrict__ tiles, uint8_t* __restrict__ clamped,
                                                    WgTotals* __restrict__ wg) {
  preprocess_block<DEG, ROW_GLOBAL>(g, c, radii, splat, binrec, depth_key, tiles, clamped, wg);
}

// The antialiased preprocess (gs_forward_preprocess_aa): k_preprocess's body with the opacity scaled.
template <int DEG>
__global__ __launch_bounds__(256) void k_preprocess_aa(GaussianArgs g, CameraArgs c, int* __restrict__ radii,
                                                       float4* __restrict__ splat, float4* __restrict__ binrec,
                                                       uint32_t* __restrict__ depth_key,
                                                       uint32_t* __restrict__ tiles, uint8_t* __restrict__ clamped,
                                                       WgTotals* __restrict__ wg) {
  preprocess_block<DEG, ROW_GLOBAL, true>(g, c, radii, splat, binrec, depth_key, tiles, clamped, wg);
}

// The split-SH preprocess: k_preprocess's body with the split row loader (ROW_SPLIT).  Five waves
// per SIMD asked for: degree 3 allocates 98 VGPRs without it (4 waves), 96 and no spill with it.
template <int DEG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_preprocess_split(
    GaussianArgs g, CameraArgs c, int* __restrict__ radii, float4* __restrict__ splat, float4* __restrict__ binrec,
    uint32_t* __restrict__ depth_key, uint32_t* __restrict__ tiles, uint8_t* __restrict__ clamped,
    WgTotals* __restrict__ wg) {
  preprocess_block<DEG, ROW_SPLIT>(g, c, radii, splat, binrec, depth_key, tiles, clamped, wg);
}


// The preprocess grid, launched whole or -- with row waits installed on this thread
// (gs_set_row_waits) -- in row chunks: before chunk k the stream waits for event k, and chunk k
// launches the workgroups whose last row lies below its end, so every row a workgroup reads is
// behind all the waits of the chunks it spans (e.g. the all-gather of a sharded optimizer step's
// row chunk, gs_view_parallel.ShardedAdam).  Same workgroups, same outputs as one launch.
template <class Launch>
static void launch_row_chunks(const GaussianArgs& g, hipStream_t st, Launch&& launch) {
  const int nb = (g.P + 255) / 256;
  RowWait w[GS_MAX_ROW_WAITS];
  const int n = take_row_waits(w, GS_MAX_ROW_WAITS);
  int b0 = 0;
  for (int k = 0; k < n && b0 < nb; k++) {
    if (w[k].ev && !stream_wait(st, w[k].ev)) return;
    const int b1 = w[k].hi >= g.P ? nb : w[k].hi / 256;
    if (b1 > b0) {
      GaussianArgs gc = g;
      gc.blk0 = b0;
      launch(gc, dim3(b1 - b0));
      b0 = b1;
    }
  }
  if (b0 < nb) {
    GaussianArgs gc = g;
    gc.blk0 = b0;
    launch(gc, dim3(nb - b0));
  }
}

void fwd_preprocess(const GaussianArgs& g0, const CameraArgs& c, int* radii, const GeomPtrs& geo, hipStream_t st,
                    bool aa) {
  launch_row_chunks(g0, st,
                    [&](const GaussianArgs& g, dim3 grid) { fwd_preprocess_grid(g, c, radii, geo, st, grid, aa); });
}

void fwd_preprocess_grid(const GaussianArgs& g, const CameraArgs& c, int* radii, const GeomPtrs& geo, hipStream_t st,
                         dim3 grid, bool aa) {
  const dim3 block(256);
  if (aa) {  // whole SH rows or colours (the entry refuses split rows)
    with_degree<-1>(g.colors ? -1 : g.D, [&](auto D) {
      GS_LAUNCH("preprocess", (k_preprocess_aa<decltype(D)::value>), grid, block, 0, st, g, c, radii, geo.splat,
                geo.binrec, geo.keys_a, geo.tiles, geo.clamped, geo.wg_tot);
    });
    return;
  }
  if (g.shs_rest && !g.colors) {  // split SH rows (M >= 2, so D >= 0 applies)
    with_degree(g.D, [&](auto D) {
      GS_LAUNCH("preprocess", (k_preprocess_split<decltype(D)::value>), grid, block, 0, st, g, c, radii, geo.splat,
                geo.binrec, geo.keys_a, geo.tiles, geo.clamped, geo.wg_tot);
    });
    return;
  }
  with_degree<-1>(g.colors ? -1 : g.D, [&](auto D) {
    GS_LAUNCH("preprocess", (k_preprocess<decltype(D)::value>), grid, block, 0, st, g, c, radii, geo.splat, geo.binrec,
              geo.keys_a, geo.tiles, geo.clamped, geo.wg_tot);
  });
}

// K views in one launch.  Every lane forms the camera-independent half of its Gaussian once
// (preprocess_shared: mean, 3D covariance, opacity and culling limit, unconditionally -- a Gaussian
// culled by one camera may be visible to the next) and then runs preprocess_view for each camera in
// turn: the code of the single-view kernels, so each view's outputs are bit-identical to its own
// launch.  The SH rows, by GS_PREVIEWS_ROWS (C3, 4 views, per launch; the parent reloaded every
// input for every view: 223 us, 122 VGPRs, 4 waves per SIMD):
//   2  (the build) loaded once per lane and held in registers across the views (ROW_REGS), every
//      layout: 126 VGPRs at degree 3, 4 waves per SIMD, 165 us
//   1  staged in LDS once per workgroup (ROW_LDS: coalesced 16-B loads; 93 VGPRs but 52 KB of LDS at
//      degree 3, so 3 workgroups per CU), where sh_rows_stageable() holds; other layouts reload the
//      row per view (ROW_GLOBAL, as the single-view kernel does): 177 us
// The per-view workgroup totals go to each view's WgTotals slots as in k_preprocess; every lane of
// the workgroup reaches both barriers of every view.
#ifndef GS_PREVIEWS_ROWS
#define GS_PREVIEWS_ROWS 2
#endif
template <int DEG, int SRC>
__global__ __launch_bounds__(256) void k_preprocess_views(GaussianArgs g, PreViews pv) {
  const int b = (int)blockIdx.x + g.blk0, i = b * 256 + (int)threadIdx.x;
  const float* lds_row = nullptr;
  if constexpr (SRC == ROW_LDS) lds_row = stage_block_rows<DEG>(g, b);
  PreShared<DEG, SRC> sh{};
  if (i < g.P) sh = preprocess_shared<DEG, SRC, true>(i, g, lds_row);
  for (int v = 0; v < pv.K; v++) {
    const GeomPtrs& geo = pv.geo[v];
    uint32_t area = 0, dbits = 0;
    bool culled = false;
    if (i < g.P) {
      area = preprocess_view<DEG, SRC, true>(i, sh, g, pv.c[v], pv.radii[v], geo.splat, geo.binrec, dbits, geo.tiles,
                                       geo.clamped, culled);
      geo.keys_a[i] = area ? dbits : DEPTH_DROP;
    }
    workgroup_totals(area, culled, geo.wg_tot, (uint32_t)b);
    lds_barrier();  // workgroup_totals' LDS is reused by the next view
  }
}

void fwd_preprocess_views(const GaussianArgs& g0, const PreViews& pv, hipStream_t st) {
  launch_row_chunks(g0, st, [&](const GaussianArgs& g, dim3 grid) {
    const dim3 block(256);
    auto launch = [&](auto D, auto SRC, size_t lds) {
      GS_LAUNCH("preprocess_views", (k_preprocess_views<decltype(D)::value, decltype(SRC)::value>), grid, block, lds, st,
                g, pv);
    };
    using std::integral_constant;
    if (g.colors) return launch(integral_constant<int, -1>{}, integral_constant<int, ROW_GLOBAL>{}, 0);
#if GS_PREVIEWS_ROWS == 1
    if (sh_rows_stageable(g.D, g.M, g.shs)) {  // degrees 1 and 3
      constexpr integral_constant<int, ROW_LDS> LDS{};
      if (g.D == 1) return launch(integral_constant<int, 1>{}, LDS, sh_stage_bytes(sh_row_floats(1)));
      return launch(integral_constant<int, 3>{}, LDS, sh_stage_bytes(sh_row_floats(3)));
    }
    constexpr int SRC = ROW_GLOBAL;
#else
    constexpr int SRC = ROW_REGS;
#endif
    with_degree(g.D, [&](auto D) { launch(D, integral_constant<int, SRC>{}, 0); });
  });
}

// ------------------------------------------------------------------------------------------
// ordering: compaction -> depth sort -> instance offsets
// ------------------------------------------------------------------------------------------

struct SrcTilesByRank {
  const uint32_t *tiles, *sorted_gid;
  uint32_t P;
  // (a depth sort whose look-back timed out leaves stale ids: stay in bounds, the forward raises)
  __device__ uint32_t operator()(uint32_t s) const {
    const uint32_t g = sorted_gid[s];
    return g < P ? tiles[g] : 0u;
  }
  __device__ SrcTilesByRank view(uint64_t vstride) const {
    return SrcTilesByRank{vptr(tiles, vstride), vptr(sorted_gid, vstride), P};
  }
};
#if GS_VIEWS_SCAN_GATHER == 4
// the batched K-view scan over the depth sort's packed values (id | min(count, PACK_MAX) <<
// PACK_ID_BITS): a saturated count is looked up; the down sweep (CLEAN) leaves the plain id behind
template <bool CLEAN>
struct SrcPackedCounts {
  const uint32_t* tiles;
  uint32_t* sorted_gid;
  uint32_t P;
  __device__ uint32_t operator()(uint32_t s) const {
    const uint32_t w = sorted_gid[s], g = w & PACK_ID_MASK, t = w >> PACK_ID_BITS;
    if constexpr (CLEAN) sorted_gid[s] = g;
    return t < PACK_MAX ? t : (g < P ? tiles[g] : 0u);
  }
  __device__ SrcPackedCounts view(uint64_t vstride) const {
    return SrcPackedCounts{vptr(tiles, vstride), vptr(sorted_gid, vstride), P};
  }
};
#endif
#if GS_VIEWS_SCAN_GATHER == 2
// the reduce sweep of the batched K-view scan: gathers like SrcTilesByRank and keeps the count at
// its rank for the down sweep (SrcArray)
struct SrcTilesByRankKeep {
  const uint32_t *tiles, *sorted_gid;
  uint32_t* by_rank;
  uint32_t P;
  __device__ uint32_t operator()(uint32_t s) const {
    const uint32_t g = sorted_gid[s];
    const uint32_t t = g < P ? tiles[g] : 0u;
    by_rank[s] = t;
    return t;
  }
  __device__ SrcTilesByRankKeep view(uint64_t vstride) const {
    return SrcTilesByRankKeep{vptr(tiles, vstride), vptr(sorted_gid, vstride), vptr(by_rank, vstride), P};
  }
};
#endif

// instance offsets in depth order; also records, for every DUP_SLOTS-aligned slot, the depth rank
// that owns it (the start of each load-balanced duplicate block)
struct DstOffsets {
  uint32_t* offsets;
  uint32_t* first;
  const uint32_t* counters;  // [CNT_NREND] I (summed by preprocess, complete before this scan runs)
  uint32_t P;
  __device__ void operator()(uint32_t s, uint32_t ex, uint32_t v) const {
    offsets[s] = ex;
    const uint32_t I = counters[CNT_NREND];
    if (!dup_balanced(I, P)) return;
    for (uint32_t m = (ex + DUP_SLOTS - 1) / DUP_SLOTS; m * DUP_SLOTS < ex + v && m * DUP_SLOTS < I; m++) first[m] = s;
  }
  __device__ DstOffsets view(uint64_t vstride) const {
    return DstOffsets{vptr(offsets, vstride), vptr(first, vstride), vptr(counters, vstride), P};
  }
};

// workgroups per tile-sort / depth-sort pass (sort_plan): one per 2048-key tile up to 8M keys
// (128 or 256 depth-sort workgroups, smaller histograms but longer scatters: 961 -> 953 / 924 it/s)
constexpr uint32_t GS_TILE_SORT_BLOCKS = 4096, GS_DEPTH_SORT_BLOCKS = 4096;
// The extra workgroup of the first depth-sort histogram launch: the view's totals from the preprocess
// workgroups' WgTotals (64-bit instance sum: an overflow of the 32-bit instance positions is seen
// exactly), written to the view's counters (which need no zeroing beforehand: every counter the
// later kernels read is set here) and to the host's readback words (host: a device-visible pointer
// into pinned host memory, or null): [0] instances low, [1] high, [2] V, [3] error flags.
struct CounterFinalize {
  static constexpr bool active = true;
  const WgTotals* wg;
  uint32_t nwg;
  uint32_t* counters;
  uint32_t* host;    // view v's words at host + 8 v
  uint32_t* sticky;  // pinned host words for a view with error flags (gs_forward_bounded), or null
  uint64_t vstride;  // bytes between the views' geometry buffers (batched launch)
  uint32_t cap[FUSED_MAX_VIEWS];  // the views' binning capacities
  __device__ void operator()(uint32_t v) const {
    const WgTotals* wg = vptr(this->wg, vstride);
    uint32_t* counters = vptr(this->counters, vstride);
    uint32_t* host = this->host ? this->host + 8 * v : nullptr;
    const uint32_t cap = this->cap[v];
    __shared__ uint32_t s_lo[4], s_hi[4], s_v[4], s_e[4];
    unsigned long long si = 0;
    uint32_t sv = 0, se = 0;
    for (uint32_t k = threadIdx.x; k < nwg; k += SORT_THREADS) {
      const WgTotals t = wg[k];
      si += t.inst;
      sv += t.vis & 0x7FFFFFFFu;
      se |= t.vis >> 31;
    }
    uint32_t lo = (uint32_t)si, hi = (uint32_t)(si >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t olo = (uint32_t)__shfl_xor((int)lo, d, 64), ohi = (uint32_t)__shfl_xor((int)hi, d, 64);
      const unsigned long long a = ((unsigned long long)hi << 32 | lo) + ((unsigned long long)ohi << 32 | olo);
      lo = (uint32_t)a;
      hi = (uint32_t)(a >> 32);
      sv += (uint32_t)__shfl_xor((int)sv, d, 64);
      se |= (uint32_t)__shfl_xor((int)se, d, 64);
    }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_lo[w] = lo, s_hi[w] = hi, s_v[w] = sv, s_e[w] = se;
    lds_barrier();
    if (threadIdx.x == 0) {
      unsigned long long I = 0;
      uint32_t V = 0, e = 0;
      for (int k = 0; k < SORT_THREADS / 64; k++) {
        I += (unsigned long long)s_hi[k] << 32 | s_lo[k];
        V += s_v[k];
        e |= s_e[k];
      }
      const uint32_t err = (e ? ERR_PREFILTERED : 0u) | (I > (unsigned long long)GS_MAX_INSTANCES ? ERR_INSTANCES : 0u) |
                           (I > (unsigned long long)cap ? ERR_CAPACITY : 0u);
      counters[CNT_NREND] = (uint32_t)I;
      counters[CNT_V] = V;
      counters[CNT_ERR] = err;
      counters[CNT_I] = 0u;
      counters[CNT_LB_TILE] = 0u;
      counters[CNT_SEQ] = counters[CNT_SEQ] + 1u;
      if (host) {
        host[0] = (uint32_t)I;
        host[1] = (uint32_t)(I >> 32);
        host[2] = V;
        host[3] = err;
      }
      if (sticky && err) {
        sticky[0] = err;
        sticky[1] = (uint32_t)I;
        sticky[2] = (uint32_t)(I >> 32);
      }
    }
  }
};

void fwd_scan(int P, const GeomPtrs& geo, hipStream_t st);

void fwd_order(int P, const GeomPtrs& geo, hipStream_t st, uint32_t* host_counts, hipEvent_t counts_ready,
               const uint32_t* cap, uint32_t* sticky, int views, uint64_t vstride) {
  const uint32_t n = (uint32_t)P;
  // the first depth-sort pass's counts, with each view's totals finalised by an extra workgroup
  // (the host waits for this launch only: the rest of the ordering overlaps its readback)
  const SortPlan sp = sort_plan(n, GS_DEPTH_SORT_BLOCKS);
  CounterFinalize fin{geo.wg_tot, (n + 255) / 256, geo.counters, host_counts, sticky, vstride, {}};
  for (int v = 0; v < FUSED_MAX_VIEWS; v++) fin.cap[v] = cap && v < views ? cap[v] : 0xFFFFFFFFu;
  GS_LAUNCH("radix_hist", k_radix_hist<CounterFinalize>, dim3(sp.nb + 1, views), dim3(SORT_THREADS), 0, st,
            geo.keys_a, nullptr, n, 0, radix_first_bits(32), sp.chunk, sp.nb, geo.sort_scratch, true, vstride, fin);
  if (counts_ready) (void)hipEventRecord(counts_ready, st);
  // depth sort of the Gaussians with instances: the first pass reads all P keys in index order
  // and drops the DEPTH_DROP ones (compaction), the later passes sort the V survivors; every
  // view's passes in one set of launches (blockIdx.y = view)
  if (lb_tiles(n) <= LB_STATIC_MAX) {
    // (GS_VIEWS_SCAN_GATHER == 3, several views: the last pass also leaves tiles[gid] at the key's rank)
    // (== 4: the first pass packs it beside the id, and the scan below unpacks it)
    const bool ranked = GS_VIEWS_SCAN_GATHER >= 3 && views > 1;
    radix_sort_pairs(geo.keys_a, geo.vals_a, geo.keys_b, geo.vals_b, true, &geo.counters[CNT_V], n, 32,
                     geo.sort_scratch, st, /*drop_first=*/true, /*hist0_ready=*/true, nullptr, nullptr, nullptr,
                     nullptr, GS_DEPTH_SORT_BLOCKS, views, vstride, ranked ? geo.tiles : nullptr,
                     ranked ? geo.rtiles_a : nullptr);
  } else {
    // larger scenes: the tile counts travel with the keys through the sort (read in index order by
    // the first pass), and the 3-launch scan reads them in depth order, coalesced (C5, 5M: the
    // per-rank gather and the ticketed look-back took 197 us)
    radix_sort_pairs(geo.keys_a, geo.vals_a, geo.keys_b, geo.vals_b, true, &geo.counters[CNT_V], n, 32,
                     geo.sort_scratch, st, /*drop_first=*/true, /*hist0_ready=*/true, geo.tiles, geo.rtiles_a,
                     geo.rtiles_b, nullptr, GS_DEPTH_SORT_BLOCKS, views, vstride);
  }
  if (views == 1) {
    fwd_scan(P, geo, st);
    return;
  }
  // several views: their offsets scans as one 3-launch scan (blockIdx.y = view; no workgroup waits
  // for another, so this scan never sets ERR_LOOKBACK and leaves counters[CNT_LB_TILE] unused)
  const DstOffsets dst{geo.offsets, geo.dup_first, geo.counters, n};
  if (lb_tiles(n) > LB_STATIC_MAX) {  // the counts travelled with the keys
    scan_exclusive(SrcArray{geo.tiles_by_rank}, dst, &geo.counters[CNT_V], n, geo.scan_partial, &geo.counters[CNT_I],
                   st, views, vstride);
    return;
  }
#if GS_VIEWS_SCAN_GATHER == 1
  scan_exclusive(SrcTilesByRank{geo.tiles, geo.sorted_gid, n}, dst, &geo.counters[CNT_V], n, geo.scan_partial,
                 &geo.counters[CNT_I], st, views, vstride);
#elif GS_VIEWS_SCAN_GATHER == 2
  scan_exclusive2(SrcTilesByRankKeep{geo.tiles, geo.sorted_gid, geo.rtiles_a, n}, SrcArray{geo.rtiles_a}, dst,
                  &geo.counters[CNT_V], n, geo.scan_partial, &geo.counters[CNT_I], st, views, vstride);
#elif GS_VIEWS_SCAN_GATHER == 4
  scan_exclusive2(SrcPackedCounts<false>{geo.tiles, geo.sorted_gid, n}, SrcPackedCounts<true>{geo.tiles, geo.sorted_gid, n},
                  dst, &geo.counters[CNT_V], n, geo.scan_partial, &geo.counters[CNT_I], st, views, vstride);
#elif GS_VIEWS_SCAN_GATHER == 3
  scan_exclusive(SrcArray{geo.rtiles_a}, dst, &geo.counters[CNT_V], n, geo.scan_partial, &geo.counters[CNT_I], st,
                 views, vstride);
#else
#error "GS_VIEWS_SCAN_GATHER: 1, 2, 3 or 4"
#endif
}

__global__ __launch_bounds__(64) void k_clear_flags(uint32_t* __restrict__ err, uint32_t bits) {
  if (threadIdx.x == 0) err[0] = err[0] & ~bits;
}
void fwd_clear_flags(const GeomPtrs& geo, uint32_t bits, hipStream_t st) {
  GS_LAUNCH("clear_flags", k_clear_flags, dim3(1), dim3(64), 0, st, &geo.counters[CNT_ERR], bits);
}

// instance offsets in depth order (+ the duplicate's block owner table), after the depth sort
void fwd_scan(int P, const GeomPtrs& geo, hipStream_t st) {
  const uint32_t n = (uint32_t)P;
  if (lb_tiles(n) <= LB_STATIC_MAX) {
    // up to 1M Gaussians: one look-back launch whose grid is resident (static tile ids); it
    // gathers each rank's tile count (cheaper here than carrying the counts through the four sort
    // passes)
    scan_exclusive_lb(SrcTilesByRank{geo.tiles, geo.sorted_gid, n}, DstOffsets{geo.offsets, geo.dup_first, geo.counters, n},
                      &geo.counters[CNT_V], n, geo.lb_status, &geo.counters[CNT_LB_TILE], &geo.counters[CNT_I],
                      &geo.counters[CNT_ERR], st, &geo.counters[CNT_SEQ]);
  } else {
    scan_exclusive(SrcArray{geo.tiles_by_rank}, DstOffsets{geo.offsets, geo.dup_first, geo.counters, n},
                   &geo.counters[CNT_V], n, geo.scan_partial, &geo.counters[CNT_I], st);
  }
}

// ------------------------------------------------------------------------------------------
// binning
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ SpanCtx span_of(const float4* __restrict__ binrec, uint32_t gid, int& y0, int& y1) {
  const float4 a = binrec[2 * gid], b = binrec[2 * gid + 1];
  const uint32_t xr = __float_as_uint(b.z), yr = __float_as_uint(b.w);
  y0 = (int)(yr & 0xFFFFu);
  y1 = (int)(yr >> 16);
  return span_ctx(a.x, a.y, a.z, a.w, b.x, b.y, (int)(xr & 0xFFFFu), (int)(xr >> 16));
}

__global__ __launch_bounds__(256) void k_duplicate(uint32_t P, const uint32_t* __restrict__ counters,
                                                   const uint32_t* __restrict__ sorted_gid,
                                                   const uint32_t* __restrict__ offsets,
                                                   const float4* __restrict__ binrec, int gx,
                                                   uint32_t* __restrict__ tile_keys,
                                                   uint32_t* __restrict__ presort_gid) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= P || s >= counters[CNT_V] || (counters[CNT_ERR] & ERR_INVALID)) return;  // (invalid list: write nothing)
  const uint32_t gid = sorted_gid[s];
  uint32_t off = offsets[s];
  // (a timed-out offsets scan only under-estimates offsets: every write stays below I)
  int y0, y1;
  const SpanCtx sp = span_of(binrec, gid, y0, y1);
  for (int ty = y0; ty < y1; ty++) {
    int ta, tb;
    row_span(sp, ty, ta, tb);
    for (int x = ta; x < tb; x++) {
      tile_keys[off] = (uint32_t)(ty * gx + x);
      presort_gid[off] = gid;
      off++;
    }
  }
}

// Load-balanced duplicate: workgroup b writes instance slots [b S, (b + 1) S), S = DUP_SLOTS.
// The depth ranks owning those slots are [dup_first[b], dup_first[b + 1]] (at most S + 1 of
// them).  Each splat's instances are its tile-exact row spans (row_span), laid out row by row;
// the row segments meeting the block are numbered with a workgroup scan, every slot finds its
// segment by an inclusive max-scan over segment start marks, and keys / presort ids are written
// fully coalesced.  The workgroups also clear the tile ranges (k_ranges fills the non-empty ones).
constexpr int DUP_THREADS = 256;
constexpr int DUP_ITEMS = DUP_SLOTS / DUP_THREADS;
// LDS index of slot i in the owner array: one pad word per 8 slots keeps the per-thread runs of
// 8 consecutive slots on distinct banks
__device__ __forceinline__ uint32_t own_idx(uint32_t i) { return i + (i >> 3); }

// Views (blockIdx.y): view v's geometry / binning / image arrays lie v * gs / bs / is bytes further.
__global__ __launch_bounds__(DUP_THREADS) void k_duplicate_lb(
    uint32_t I, const uint32_t* __restrict__ counters, const uint32_t* __restrict__ dup_first,
    const uint32_t* __restrict__ sorted_gid, const uint32_t* __restrict__ offsets,
    const float4* __restrict__ binrec, int gx, int gy, uint32_t* __restrict__ tile_keys,
    uint32_t* __restrict__ presort_gid, uint2* __restrict__ ranges, uint32_t* __restrict__ hist0, uint32_t mask0,
    uint32_t* __restrict__ n_copy, uint64_t gs, uint64_t bs, uint64_t is) {
  counters = vptr(counters, gs), dup_first = vptr(dup_first, gs), sorted_gid = vptr(sorted_gid, gs);
  offsets = vptr(offsets, gs), binrec = vptr(binrec, gs);
  tile_keys = vptr(tile_keys, bs), presort_gid = vptr(presort_gid, bs), hist0 = vptr(hist0, bs);
  n_copy = vptr(n_copy, bs), ranges = vptr(ranges, is);
  __shared__ uint32_t s_own[DUP_SLOTS + DUP_SLOTS / 8];  // (slot + 1) << 16 | segment at segment starts
  // per row segment: (tile id of its first slot) - (that slot), mod 2^32 (the slot may precede the
  // block), so slot k of the segment has key base + k; one table instead of two keeps the LDS at
  // 26 KB: 6 workgroups per CU
  __shared__ uint32_t s_seg_base[DUP_SLOTS];
  __shared__ uint32_t s_seg_gid[DUP_SLOTS];
  __shared__ uint32_t s_wmax[DUP_THREADS / 64];
  __shared__ uint32_t s_nseg;
  __shared__ uint32_t s_hist[RADIX];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  s_hist[tid] = 0;
  const uint32_t tiles = (uint32_t)(gx * gy);
  for (uint32_t t = b * DUP_THREADS + tid; t < tiles; t += gridDim.x * DUP_THREADS) ranges[t] = make_uint2(0u, 0u);
  const uint32_t V = counters[CNT_V];
  // I: the binning buffer's capacity (= the count, unless the buffer was sized ahead of it)
  I = min(I, counters[CNT_NREND]);
  if (b == 0 && tid == 0) n_copy[0] = I;  // for the tile sort and k_ranges (kernels after this one)
  const uint32_t k0 = b * DUP_SLOTS;
  const uint32_t k1 = k0 < I ? min(k0 + DUP_SLOTS, I) : k0;
  if (counters[CNT_ERR] & ERR_INVALID) {
    // a look-back wait of the depth sort or the offsets scan timed out, or the instances exceed the
    // buffer (the host raises at its next call): the owner table is not valid, so fill the block's
    // slots with a safe placeholder -- tile 0, Gaussian 0 -- that keeps every later kernel in bounds
    const uint32_t g0 = 0u;
    for (uint32_t k = k0 + tid; k < k1; k += DUP_THREADS) {
      tile_keys[k] = 0u;
      presort_gid[k] = g0;
    }
    if (hist0) {
      hist0[(size_t)tid * gridDim.x + b] = tid == 0 ? k1 - k0 : 0u;
    }
    return;
  }
  if (k1 == k0) {  // past the count (a buffer sized ahead of it): no slots
    if (hist0) hist0[(size_t)tid * gridDim.x + b] = 0u;
    return;
  }
  const uint32_t s_lo = dup_first[b];
  const uint32_t s_hi = (k1 < I) ? dup_first[b + 1] : V - 1;
  const uint32_t nG = s_hi - s_lo + 1;
  for (uint32_t i = tid; i < DUP_SLOTS + DUP_SLOTS / 8; i += DUP_THREADS) s_own[i] = 0;
  if (tid == 0) s_nseg = 0;
  lds_barrier();
  // row segments of the block's splats that meet [k0, k1): any segment numbering works, the
  // marks carry their slot so the scan below picks the segment that starts last at or before
  // each slot (deterministic output)
  for (uint32_t r = tid; r < nG; r += DUP_THREADS) {
    const uint32_t gid = sorted_gid[s_lo + r];
    uint32_t pos = offsets[s_lo + r];
    if (pos >= k1) continue;
    int y0, y1;
    const SpanCtx sp = span_of(binrec, gid, y0, y1);
    for (int ty = y0; ty < y1 && pos < k1; ty++) {
      int ta, tb;
      row_span(sp, ty, ta, tb);
      const uint32_t w = (uint32_t)(tb - ta);
      if (w && pos + w > k0) {
        const uint32_t seg = atomicAdd(&s_nseg, 1u);
        s_seg_base[seg] = (uint32_t)(ty * gx + ta) - pos;
        s_seg_gid[seg] = gid;
        const uint32_t at = (pos > k0 ? pos : k0) - k0;
        s_own[own_idx(at)] = ((at + 1) << 16) | seg;
      }
      pos += w;
    }
  }
  lds_barrier();
  // inclusive max-scan of the marks over the block's slots (consecutive DUP_ITEMS per thread)
  uint32_t v[DUP_ITEMS];
  uint32_t run = 0;
#pragma unroll
  for (int r = 0; r < DUP_ITEMS; r++) {
    run = max(run, s_own[own_idx(tid * DUP_ITEMS + r)]);
    v[r] = run;
  }
  uint32_t incl = run;
  const uint32_t lane = tid & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= (uint32_t)d) incl = max(incl, o);
  }
  if (lane == 63) s_wmax[tid >> 6] = incl;
  uint32_t excl = (uint32_t)__shfl_up((int)incl, 1, 64);
  if (lane == 0) excl = 0;
  lds_barrier();
  for (uint32_t w = 0; w < (tid >> 6); w++) excl = max(excl, s_wmax[w]);
#pragma unroll
  for (int r = 0; r < DUP_ITEMS; r++) s_own[own_idx(tid * DUP_ITEMS + r)] = max(v[r], excl);
  lds_barrier();
#pragma unroll
  for (int r = 0; r < DUP_ITEMS; r++) {
    const uint32_t i = (uint32_t)r * DUP_THREADS + tid;
    const uint32_t k = k0 + i;
    if (k < k1) {
      const uint32_t o = s_own[own_idx(i)] & 0xFFFFu;
      const uint32_t key = s_seg_base[o] + k;
      tile_keys[k] = key;
      presort_gid[k] = s_seg_gid[o];
      if (hist0) atomicAdd(&s_hist[key & mask0], 1u);  // counts only: order-free
    }
  }
  // the tile sort's first-pass digit counts of this block's slots (its sort tile is the same 2048
  // slots): the sort skips that pass's counting launch
  if (hist0) {
    lds_barrier();
    hist0[(size_t)tid * gridDim.x + b] = s_hist[tid];
  }
}

// tile ranges over the sorted instance list, 4 instances per lane
__global__ __launch_bounds__(256) void k_ranges(uint32_t I, const uint32_t* __restrict__ n_dev,
                                                const uint32_t* __restrict__ tile, uint2* __restrict__ ranges,
                                                uint32_t* __restrict__ sched, uint32_t n_sched, uint32_t tiles,
                                                uint64_t bs, uint64_t is) {
  n_dev = vptr(n_dev, bs), tile = vptr(tile, bs), ranges = vptr(ranges, is), sched = vptr(sched, is);
  // clear the render's per-tile completion words and the backward queue (k_render_fwd_q epilogue)
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_sched; i += gridDim.x * 256) sched[i] = 0u;
  I = min(I, *n_dev);  // the capacity I, or the count when below it
  const uint32_t k0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k0 >= I) return;
  uint32_t t[6];
  t[0] = k0 > 0 ? tile[k0 - 1] : 0xFFFFFFFFu;
  if (k0 + 4 <= I && (k0 & 3) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(tile + k0);
    t[1] = q.x;
    t[2] = q.y;
    t[3] = q.z;
    t[4] = q.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; r++) t[1 + r] = k0 + r < I ? tile[k0 + r] : 0xFFFFFFFFu;
  }
  t[5] = k0 + 4 < I ? tile[k0 + 4] : 0xFFFFFFFFu;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint32_t k = k0 + r;
    if (k >= I) break;
    if (t[r + 1] >= tiles) continue;  // only after a timed-out sort (reported): stay in bounds
    if (t[r + 1] != t[r]) ranges[t[r + 1]].x = k;
    if (t[r + 2] != t[r + 1]) ranges[t[r + 1]].y = k + 1;
  }
}

// Tile ranges of the packed tile sort, without the sorted keys: one lane per tile t = (h, l), l its
// low fb bits.  The second pass sorted the padded first-pass output, in which low digit l's region
// covers the whole workgroups [tab[l], tab[l + 1]); its row-scanned histogram off2[h][b] counts the
// words of high digit h in the workgroups before b, so tile t's instances are
// base2[h] + [off2[h][tab[l]], off2[h][tab[l + 1]]) (a workgroup index at nb2: the row total).
// Also clears the scheduling words, like k_ranges.
__global__ __launch_bounds__(256) void k_ranges_packed(const uint32_t* __restrict__ off2,
                                                       const uint32_t* __restrict__ row_total2, uint32_t nb2,
                                                       const uint32_t* __restrict__ tab, int fb,
                                                       uint2* __restrict__ ranges, uint32_t* __restrict__ sched,
                                                       uint32_t n_sched, uint32_t tiles, uint64_t bs, uint64_t is) {
  __shared__ uint32_t s_scan[4];
  __shared__ uint32_t s_base2[RADIX], s_tot2[RADIX];
  off2 = vptr(off2, bs), row_total2 = vptr(row_total2, bs), tab = vptr(tab, bs);
  ranges = vptr(ranges, is), sched = vptr(sched, is);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_sched; i += gridDim.x * 256) sched[i] = 0u;
  const uint32_t rt = row_total2[threadIdx.x];
  uint32_t all;
  s_base2[threadIdx.x] = block_excl_scan(rt, s_scan, &all);
  s_tot2[threadIdx.x] = rt;
  lds_barrier();
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= tiles) return;
  const uint32_t h = t >> fb, l = t & ((1u << fb) - 1u);
  const uint32_t b0 = tab[l], b1 = tab[l + 1];
  const uint32_t* row = off2 + (size_t)h * nb2;
  const uint32_t x = b0 < nb2 ? row[b0] : s_tot2[h], y = b1 < nb2 ? row[b1] : s_tot2[h];
  ranges[t] = x < y ? make_uint2(s_base2[h] + x, s_base2[h] + y) : make_uint2(0u, 0u);
}

// The packed two-pass tile sort: (tile, slot) as one word after the first pass, no key output from
// the second, ranges from the second pass's histogram (k_ranges_packed).  It runs for two-pass
// sorts (9 .. 16 tile bits) whose high digit and slot fit 32 bits, when the padded first-pass output
// -- up to 2^fb chunks more than the I instances -- fits the 2 I words of keys_b | vals_b, both
// unused by this path.  Everything else takes radix_sort_pairs + k_ranges.
struct PackedPlan {
  int fb, hb;
  uint32_t sb;      // bits of the slot field: I < 2^sb
  SortPlan p1;      // first pass, over the I slots
  uint32_t n2_max;  // words of the padded intermediate
  uint32_t nb2;     // second-pass workgroups (of p1.chunk words)
};
static bool packed_plan(uint32_t I, int tbits, PackedPlan* pp) {
  if (radix_passes(tbits) != 2) return false;
  pp->fb = radix_first_bits(tbits), pp->hb = tbits - pp->fb;
  pp->sb = 1;
  while (pp->sb < 32 && ((uint64_t)1 << pp->sb) <= (uint64_t)I) pp->sb++;
  if ((uint32_t)pp->hb + pp->sb > 32) return false;
  pp->p1 = sort_plan(I, GS_TILE_SORT_BLOCKS);
  const uint64_t pad = (uint64_t)pp->p1.chunk << pp->fb;
  // (32-bit positions: a position plus one chunk stays below 2^32)
  if (pad > (uint64_t)I || (uint64_t)I + pad + pp->p1.chunk >= ((uint64_t)1 << 32)) return false;
  pp->n2_max = (uint32_t)(I + pad);
  pp->nb2 = (pp->n2_max + pp->p1.chunk - 1) / pp->p1.chunk;  // = p1.nb + 2^fb <= the scratch's columns
  return true;
}

static void tile_sort_packed_views(int views, uint32_t I, const PackedPlan& pp, bool hist0, const BinPtrs& bin,
                                   const ImgPtrs& img, uint32_t tiles, uint32_t sched_n, uint64_t bs, uint64_t is,
                                   hipStream_t st) {
  const SortPlan& p = pp.p1;
  uint32_t* hist = bin.sort_scratch;
  uint32_t* padded = bin.keys_b;  // keys_b | vals_b
  const PackArgs pk{pp.sb, bin.pack_tab};
  if (!hist0)
    GS_LAUNCH("radix_hist", k_radix_hist<NoFin>, dim3(p.nb, views), dim3(SORT_THREADS), 0, st, bin.slot_tile,
              bin.count, I, 0, pp.fb, p.chunk, p.nb, hist, false, bs, NoFin());
  uint32_t* row_total = hist + (size_t)RADIX * p.nb;
  GS_LAUNCH("radix_rowscan", k_radix_rowscan<>, dim3(RADIX, views), dim3(SORT_THREADS), 0, st, hist, p.nb, row_total,
            bs);
  auto with_bits = [](int bits, auto&& f) {
    switch (bits) {
      case 8: return f(std::integral_constant<int, 8>{});
      case 7: return f(std::integral_constant<int, 7>{});
      case 6: return f(std::integral_constant<int, 6>{});
      case 5: return f(std::integral_constant<int, 5>{});
      default: return f(std::integral_constant<int, 4>{});
    }
  };
  with_bits(pp.fb, [&](auto B) {
    GS_LAUNCH("radix_scatter", (k_radix_scatter<false, decltype(B)::value, 3>), dim3(p.nb, views), dim3(SORT_THREADS),
              0, st, bin.slot_tile, nullptr, padded, nullptr, bin.count, I, 0, p.chunk, p.nb, hist, row_total, false,
              nullptr, nullptr, bs, pk);
  });
  // second pass: the padded words, bounded by the padded total (device)
  const uint32_t* n2 = bin.pack_tab + PACK_TAB_TOTAL;
  GS_LAUNCH("radix_hist", k_radix_hist<NoFin>, dim3(pp.nb2, views), dim3(SORT_THREADS), 0, st, padded, n2, pp.n2_max,
            (int)pp.sb, pp.hb, p.chunk, pp.nb2, hist, true, bs, NoFin());
  row_total = hist + (size_t)RADIX * pp.nb2;
  GS_LAUNCH("radix_rowscan", k_radix_rowscan<>, dim3(RADIX, views), dim3(SORT_THREADS), 0, st, hist, pp.nb2, row_total,
            bs);
  with_bits(pp.hb, [&](auto B) {
    if constexpr (decltype(B)::value >= 5)  // (hb >= 5: two-pass sorts start at 4 + 5 bits)
      GS_LAUNCH("radix_scatter", (k_radix_scatter<false, decltype(B)::value, 4>), dim3(pp.nb2, views),
                dim3(SORT_THREADS), 0, st, padded, nullptr, nullptr, bin.point_list, n2, pp.n2_max, (int)pp.sb, p.chunk,
                pp.nb2, hist, row_total, true, nullptr, nullptr, bs, pk);
  });
  GS_LAUNCH("ranges", k_ranges_packed, dim3((tiles + 255) / 256, views), dim3(256), 0, st, hist, row_total, pp.nb2,
            bin.pack_tab, pp.fb, img.ranges, (uint32_t*)img.tile_done, sched_n, tiles, bs, is);
  tile_sort_packed_note();
}

void fwd_bin(int P, uint32_t I, const CameraArgs& c, const int* radii, const GeomPtrs& geo, const BinPtrs& bin,
             const ImgPtrs& img, hipStream_t st) {
  (void)radii;
  fwd_bin_views(1, P, I, c, geo, bin, img, 0, 0, 0, st);
}

void fwd_bin_views(int views, int P, uint32_t I, const CameraArgs& c, const GeomPtrs& geo, const BinPtrs& bin,
                   const ImgPtrs& img, uint64_t gs, uint64_t bs, uint64_t is, hipStream_t st) {
  const int tiles = c.gx * c.gy;
  const uint32_t sched_n = sched_words((uint32_t)tiles);
  if (I == 0 || !dup_balanced(I, (uint32_t)P)) {
    // no instances (capacity 0), or more than DUP_SLOTS per Gaussian on average: view by view
    for (int v = 0; v < views; v++) {
      GeomPtrs g;
      BinPtrs bb;
      ImgPtrs im;
      geom_layout((size_t)P, &g, (char*)geo.splat + (uint64_t)v * gs);
      bin_layout((size_t)I, tiles, &bb, (char*)bin.keys_a + (uint64_t)v * bs);
      img_layout(c.W, c.H, &im, (char*)img.ranges + (uint64_t)v * is);
      if (I == 0) {
        (void)hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)tiles, st);
        (void)hipMemsetAsync(im.tile_done, 0, sizeof(uint32_t) * sched_n, st);
        continue;
      }
      (void)hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)tiles, st);
      GS_LAUNCH("duplicate", k_duplicate, dim3((P + 255) / 256), dim3(256), 0, st, (uint32_t)P, g.counters,
                g.sorted_gid, g.offsets, g.binrec, c.gx, bb.slot_tile, bb.presort_gid);
      radix_sort_pairs(bb.keys_a, bb.vals_a, bb.keys_b, bb.vals_b, true, &g.counters[CNT_NREND], I, tile_bits(tiles),
                       bb.sort_scratch, st, false, false, nullptr, nullptr, nullptr, bb.slot_tile,
                       GS_TILE_SORT_BLOCKS);
      GS_LAUNCH("ranges", k_ranges, dim3((I + 1023) / 1024), dim3(256), 0, st, I, &g.counters[CNT_NREND],
                bb.sorted_tile, im.ranges, (uint32_t*)im.tile_done, sched_n, (uint32_t)tiles, 0ull, 0ull);
    }
    return;
  }
  const int tbits = tile_bits(tiles);
  // one duplicate block per sort tile: the duplicate also counts the first sort pass's digits; it
  // copies each view's bounded count into its binning buffer (bin.count) for the sort and ranges
  const bool hist0 = sort_plan(I, GS_TILE_SORT_BLOCKS).chunk == DUP_SLOTS;
  GS_LAUNCH("duplicate", k_duplicate_lb, dim3((I + DUP_SLOTS - 1) / DUP_SLOTS, views), dim3(DUP_THREADS), 0, st, I,
            geo.counters, geo.dup_first, geo.sorted_gid, geo.offsets, geo.binrec, c.gx, c.gy, bin.slot_tile,
            bin.presort_gid, img.ranges, hist0 ? bin.sort_scratch : nullptr, (1u << radix_first_bits(tbits)) - 1u,
            bin.count, gs, bs, is);
  PackedPlan pp;
  if (tile_sort_packed() && packed_plan(I, tbits, &pp)) {
    tile_sort_packed_views(views, I, pp, hist0, bin, img, (uint32_t)tiles, sched_n, bs, is, st);
    return;
  }
  // the device count bounds the sort (I is the buffers' capacity, which may exceed it)
  radix_sort_pairs(bin.keys_a, bin.vals_a, bin.keys_b, bin.vals_b, true, bin.count, I, tbits, bin.sort_scratch, st,
                   false, hist0, nullptr, nullptr, nullptr, bin.slot_tile,
                   GS_TILE_SORT_BLOCKS, views, bs);
  GS_LAUNCH("ranges", k_ranges, dim3((I + 1023) / 1024, views), dim3(256), 0, st, I, bin.count, bin.sorted_tile,
            img.ranges, (uint32_t*)img.tile_done, sched_n, (uint32_t)tiles, bs, is);
}

// ------------------------------------------------------------------------------------------
// render forward
// ------------------------------------------------------------------------------------------
// Entries are staged as three 16-B LDS records at one byte offset o (o, o + 16 NB, o + 32 NB for
// a batch of NB entries):
//   (x, y, r, g) | falloff coefficients + opacity | (b, bits(entry index + 1), AUX: 1 / z, -)
// and each quadrant wave's dense list holds the offsets (u32), read FWD_ILP = 4 at a time with one
// 16-B LDS read: a list entry costs no address arithmetic, no unpacking and no dependent list read.
// (8 entries per trip: 60 -> 74 VGPRs, 8 -> 6 waves per SIMD, render_fwd 174 -> 189 us)
constexpr int FWD_ILP = 4;  // a multiple of 4 (whole 16-B list reads)
static_assert(FWD_ILP % 4 == 0, "list groups are read 16 B at a time");

struct FwdPix {
  float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
  float D = 0.0f;  // AUX: expected inverse depth, one more colour channel of colour 1 / z (else unused)
  uint32_t last = 0;
  uint64_t done;  // lane mask (wave-uniform): pixels that stopped or lie outside the image
};

// Walk one quadrant wave's list of qcnt staged entries for the lane's pixel.  The list is padded
// with 2 FWD_ILP offsets of a staged dummy entry of opacity 0 (alpha 0 at every pixel), so the walk
// needs no per-entry end-of-list test (175.8 -> 172.6 us at C3).
// AUX (the aux outputs, gs_forward_render_aux): the entry's 1 / z rides in word 2 of its third
// record and is composited into px.D in the form and order of a colour channel.
template <bool EXACT, int NB, bool AUX = false>
__device__ __forceinline__ void fwd_walk(const char* ent, const uint32_t* qlist, uint32_t qcnt, float pfx, float pfy,
                                         FwdPix& px) {
  // FWD_ILP entries per trip: their power / exp / alpha chains are independent (ILP); the
  // compositing is then applied entry by entry in list order, exactly as one at a time.  The
  // next group's offsets are read one trip ahead (one dependent LDS round trip per trip).
  constexpr int NQ = FWD_ILP / 4;
  uint4 wn[NQ];
#pragma unroll
  for (int r = 0; r < NQ; r++) wn[r] = *reinterpret_cast<const uint4*>(&qlist[4 * r]);
  for (uint32_t k = 0; k < qcnt; k += FWD_ILP) {
    uint32_t o[FWD_ILP];
#pragma unroll
    for (int r = 0; r < NQ; r++) {
      o[4 * r] = wn[r].x, o[4 * r + 1] = wn[r].y, o[4 * r + 2] = wn[r].z, o[4 * r + 3] = wn[r].w;
      wn[r] = *reinterpret_cast<const uint4*>(&qlist[k + FWD_ILP + 4 * r]);
    }
    float pw[FWD_ILP], al[FWD_ILP];
#pragma unroll
    for (int u = 0; u < FWD_ILP; u++) {
      const float4 xr = *reinterpret_cast<const float4*>(ent + o[u]);
      const float4 co = *reinterpret_cast<const float4*>(ent + o[u] + 16 * NB);
      pw[u] = falloff_log2_m<EXACT>(co, xr.x - pfx, xr.y - pfy);  // log2(e) * power (fast: + log2 o)
      al[u] = fminf(0.99f, opac_gauss<EXACT>(co, pw[u]));
    }
#pragma unroll
    for (int u = 0; u < FWD_ILP; u++) {
      const float4 xr = *reinterpret_cast<const float4*>(ent + o[u]);
      using Rec2 = typename std::conditional<AUX, float4, float2>::type;
      const Rec2 bl = *reinterpret_cast<const Rec2*>(ent + o[u] + 32 * NB);
      const float rr = xr.z, rg = xr.w, rb = bl.x;
      float rd = 0.0f;
      if constexpr (AUX) rd = bl.z;
      // branch-free compositing (selects instead of divergent ifs); the per-entry decisions are
      // lane masks combined on the scalar unit (ballot / inverse ballot), so the VALU does the
      // two threshold compares and the selects only.
      // upstream skips power > 0; with a positive-definite conic that only happens by rounding
      // within ~1e-3 px of a splat centre, so the fast mode leaves the test out (the backward
      // matches it entry for entry)
      const uint64_t m_a = __builtin_amdgcn_ballot_w64((!EXACT || pw[u] <= 0.0f) && al[u] >= 1.0f / 255.0f);
      uint64_t m_cu = m_a & ~px.done;
      if constexpr (EXACT) {  // upstream's order, T (1 - alpha) and (rgb alpha) T, mirrored by the oracle
        const float tT = px.T * (1.0f - al[u]);
        // T would drop below 1e-4: stop before this entry
        const uint64_t m_stop = m_cu & __builtin_amdgcn_ballot_w64(tT < 0.0001f);
        px.done |= m_stop;
        m_cu &= ~m_stop;
        const bool cu = __builtin_amdgcn_inverse_ballot_w64(m_cu);
        px.C0 = cu ? px.C0 + rr * al[u] * px.T : px.C0;
        px.C1 = cu ? px.C1 + rg * al[u] * px.T : px.C1;
        px.C2 = cu ? px.C2 + rb * al[u] * px.T : px.C2;
        if constexpr (AUX) px.D = cu ? px.D + rd * al[u] * px.T : px.D;
        px.T = cu ? tT : px.T;
        px.last = cu ? __float_as_uint(bl.y) : px.last;
      } else {
        // T - alpha T as one FMA (one rounding of T (1 - alpha)); one weight, three FMAs (a
        // skipped entry adds rgb * 0)
        const float tT = __builtin_fmaf(-al[u], px.T, px.T);
        const uint64_t m_keep = __builtin_amdgcn_ballot_w64(tT >= 0.0001f);
        px.done |= m_cu & ~m_keep;
        m_cu &= m_keep;
        const bool cu = __builtin_amdgcn_inverse_ballot_w64(m_cu);
        const float wgt = cu ? al[u] * px.T : 0.0f;
        px.C0 = __builtin_fmaf(rr, wgt, px.C0);
        px.C1 = __builtin_fmaf(rg, wgt, px.C1);
        px.C2 = __builtin_fmaf(rb, wgt, px.C2);
        if constexpr (AUX) px.D = __builtin_fmaf(rd, wgt, px.D);
        px.T = cu ? tT : px.T;
        px.last = cu ? __float_as_uint(bl.y) : px.last;
      }
    }
    if (px.done == ~0ull) break;
  }
}

#ifdef GS_TIMING
// diagnostic build only: per quadrant wave b (blockIdx.x): tile << 32 | quadrant, batches staged <<
// 32 | entries walked (tools/fwd_timing.py)
GS_TIMING_BUFFER(g_fwd_timing, gs_debug_fwd_timing)
#endif

// Epilogue of one quadrant wave (one lane): one 64-bit atomic per wave adds 1 (finished waves, low
// 3 bits) plus a one-hot bit of the quadrant's walk-length class (bit 8 + class).  The tile's
// fourth finisher gets the other three from the returned value, with no fence: the highest set
// bit of the sum is the tile's longest class (or one above it, when classes coincide and carry),
// which is all the longest-first order needs.  It takes a rank in that bucket; k_tile_order turns
// (bucket, rank) into the backward's launch order.
__device__ __forceinline__ void tile_finish(uint32_t tile, uint32_t grp, uint32_t wave_last,
                                            uint64_t* __restrict__ tile_done, uint32_t* __restrict__ len_hist,
                                            uint32_t* __restrict__ tile_brank) {
  // length classes on a log scale, four per octave
  const uint32_t cls = min((uint32_t)(4.0f * __log2f((float)wave_last + 1.0f)), 47u);
  const uint64_t mine = (1ull << (8 + cls)) + 1ull;
  const uint64_t old = atomicAdd((unsigned long long*)&tile_done[tile], (unsigned long long)mine);
  if ((old & 7ull) != 3ull) return;
  const uint32_t top = 63u - (uint32_t)__builtin_clzll((old + mine) >> 8);  // 0 .. 49
  const uint32_t b = (uint32_t)ORDER_BUCKETS - 1u - top;                    // descending length
  tile_brank[tile] = b << 22 | atomicAdd(&len_hist[grp * ORDER_BUCKETS + b], 1u);
}

__device__ __forceinline__ void fwd_store(const CameraArgs& c, const QuadPix& q, bool inside, const FwdPix& px,
                                          float* __restrict__ out, float* __restrict__ final_T,
                                          uint32_t* __restrict__ n_contrib) {
  if (inside) {
    const size_t pix = (size_t)q.py * c.W + q.px, HW = (size_t)c.W * c.H;
    final_T[pix] = px.T;
    n_contrib[pix] = px.last;
    out[pix] = px.C0 + px.T * c.bg[0];
    out[HW + pix] = px.C1 + px.T * c.bg[1];
    out[2 * HW + pix] = px.C2 + px.T * c.bg[2];
  }
}
// the aux outputs of the pixel: no background term; alpha is 1 - final_T as stored (0 for a pixel
// with no contributor: T is still 1)
__device__ __forceinline__ void fwd_store_aux(const CameraArgs& c, const QuadPix& q, bool inside, const FwdPix& px,
                                              float* __restrict__ out_invdepth, float* __restrict__ out_alpha) {
  if (inside) {
    const size_t pix = (size_t)q.py * c.W + q.px;
    if (out_invdepth) out_invdepth[pix] = px.D;
    if (out_alpha) out_alpha[pix] = 1.0f - px.T;
  }
}

// One wave per (tile, quadrant), no workgroup barriers: each wave stages the tile's entries 64 at
// a time, culls them to its own quadrant and walks them, and finishes as soon as its 64 pixels
// are done (a workgroup per tile would wait for its slowest quadrant: 203 -> 188 us at C3 when this
// went in).  Workgroup b takes the (b / 32)-th tile of XCD group b % 8 (xcd_tile), quadrant
// (b / 8) % 4, so the four quadrant waves of a tile share the workgroup-to-XCD round robin (b % 8)
// and their repeated entry loads hit one L2.
// (Tried and not kept: the next batch's ids / records prefetched one batch ahead, 168 -> 179 us --
// the loads past the stop are wasted; 32-entry batches, 174 -> 195 us.)
constexpr int FWDQ_NB = 64;  // entries staged per round (one per lane)
// record stride of the staged batch: one more than the batch for the padding's dummy entry
constexpr int FWDQ_NBS = FWDQ_NB + 1;
template <bool EXACT, bool AUX = false>
__global__ __launch_bounds__(64) void k_render_fwd_q(CameraArgs c, const uint2* __restrict__ ranges,
                                                     const uint32_t* __restrict__ point_list,
                                                     const uint32_t* __restrict__ point_gid,
                                                     const float4* __restrict__ splat, float* __restrict__ out,
                                                     ImgPtrs img, const uint32_t* __restrict__ err,
                                                     uint32_t* __restrict__ err_host, FwdAux aux) {
  __shared__ float4 s_ent[3 * FWDQ_NBS];
  __shared__ __attribute__((aligned(16))) uint32_t s_qlist[FWDQ_NB + 2 * FWD_ILP];
  if (threadIdx.x < 3)  // the dummy entry: position 0, opacity 0 (never contributes; fast: log2 0 = -inf)
    s_ent[threadIdx.x * FWDQ_NBS + FWDQ_NB] =
        make_float4(0.0f, 0.0f, 0.0f, (EXACT || threadIdx.x != 1) ? 0.0f : -__builtin_inff());
  const uint32_t b = blockIdx.x;
  const uint32_t tile = xcd_tile(b & 7, b >> 5, c.gx, c.gy);
  if (tile == ~0u) return;  // (grid padded to whole groups of 8 tiles)
#ifdef GS_TIMING
  const unsigned long long t_start = timing_stamp();
  uint32_t t_batches = 0, t_walked = 0;
#endif
  const int wid = (int)((b >> 3) & 3);
  const int tx = (int)(tile % (uint32_t)c.gx), ty = (int)(tile / (uint32_t)c.gx);
  const int lane = threadIdx.x;
  // the ordering's error flags (final once the binning kernels are done) -> the host's readback word
  if (b == 0 && lane == 0 && err_host && *err) err_host[0] = *err;
  const QuadPix q = quad_pixel(tx, ty, wid, lane);
  const bool inside = q.px < c.W && q.py < c.H;
  const uint2 range = ranges[tile];
  // a sort / scan look-back that timed out (reported by the host) leaves no valid list: render none
  const uint32_t n = (*err & ERR_INVALID) ? 0u : range.y - range.x;
  const char* ent = reinterpret_cast<const char*>(s_ent);
  const float qx = (float)(tx * GS_TILE + 8 * (wid & 1)), qy = (float)(ty * GS_TILE + 8 * (wid >> 1));
  FwdPix px;
  px.done = __builtin_amdgcn_ballot_w64(!inside);
  for (uint32_t base = 0; base < n; base += FWDQ_NB) {
    if (px.done == ~0ull) break;
    bool meets = false;
    if (lane < (uint32_t)FWDQ_NB && base + lane < n) {
      const uint32_t gid = point_gid[point_list[range.x + base + lane]];
      const float4 a = splat[3 * gid], bb = splat[3 * gid + 1], d = splat[3 * gid + 2];
      s_ent[lane] = make_float4(a.x, a.y, bb.z, bb.w);
      s_ent[FWDQ_NBS + lane] = fall_coefs_m<EXACT>(a.z, a.w, bb.x, bb.y);
      // (AUX: one correctly rounded division per staged entry; z > 0.2)
      s_ent[2 * FWDQ_NBS + lane] =
          make_float4(d.x, __uint_as_float(base + lane + 1), AUX ? 1.0f / d.y : 0.0f, 0.0f);
      meets = d.z >= 0.0f && ellipse_meets_rect(a.x, a.y, a.z, a.w, bb.x, d.z, qx, qx + 7.0f, qy, qy + 7.0f);
    }
    const uint64_t m = __ballot(meets);
    if (meets)
      s_qlist[__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] =
          16u * lane;
    const uint32_t qcnt = (uint32_t)__popcll(m);
    if (lane < 2 * FWD_ILP) s_qlist[qcnt + lane] = 16u * FWDQ_NB;
    __builtin_amdgcn_wave_barrier();
#ifdef GS_TIMING
    t_batches++;
    t_walked += qcnt;
#endif
    fwd_walk<EXACT, FWDQ_NBS, AUX>(ent, s_qlist, qcnt, (float)q.px, (float)q.py, px);
    __builtin_amdgcn_wave_barrier();  // the next round overwrites the staged entries
  }
  fwd_store(c, q, inside, px, out, img.final_T, img.n_contrib);
  if constexpr (AUX) fwd_store_aux(c, q, inside, px, aux.invdepth, aux.alpha);
  const uint32_t wmax = wave_max_u32(px.last);
  if (lane == 0) {
    img.tile_max[4 * tile + wid] = wmax;
    tile_finish(tile, tile % ORDER_GROUPS, wmax, img.tile_done, img.len_hist, img.tile_brank);
  }
#ifdef GS_TIMING
  timing_record(g_fwd_timing, t_start, tile, (uint32_t)wid | n << 2, t_batches, t_walked);
#endif
}

void fwd_render(const CameraArgs& c, const GeomPtrs& geo, const BinPtrs& bin, const ImgPtrs& img, float* out_color,
                hipStream_t st, uint32_t* err_host, const FwdAux& aux) {
  const int tiles = c.gx * c.gy;
  const int blocks = (int)xcd_span((uint32_t)tiles) * 32;
  // the aux outputs: the AUX walk (gs_forward_render_aux)
  with_flag(aux.invdepth || aux.alpha, [&](auto AUX) {
    with_flag(exact_exp(), [&](auto EXACT) {
      GS_LAUNCH(decltype(AUX)::value ? "render_fwd_aux" : "render_fwd",
                (k_render_fwd_q<decltype(EXACT)::value, decltype(AUX)::value>), dim3(blocks), dim3(64), 0, st, c,
                img.ranges, bin.point_list, bin.presort_gid, geo.splat, out_color, img, &geo.counters[CNT_ERR], err_host,
                aux);
    });
  });
}

// ------------------------------------------------------------------------------------------
// mark_visible (upstream checkFrustum: near-plane test, prefiltered = false)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mark_visible(int P, const float* __restrict__ means,
                                                      const float* __restrict__ view, uint8_t* __restrict__ present) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float3v pv = xf43(view, means[3 * i], means[3 * i + 1], means[3 * i + 2]);
  present[i] = !(pv.z <= 0.2f);
}

void mark_visible(int P, const float* means3D, const float* view, const float* proj, uint8_t* present,
                  hipStream_t st) {
  (void)proj;
  if (P <= 0) return;
  GS_LAUNCH("mark_visible", k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, st, P, means3D, view, present);
}

}  // namespace gs
