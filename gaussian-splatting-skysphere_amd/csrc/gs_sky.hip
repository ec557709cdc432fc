// gs_sky.hip -- skysphere background: a learnable equirectangular texture [3, Hs, Ws], sampled per
// pixel along the camera ray and composited behind the splats, image = color + (1 - alpha) sky.
//
// Pixel (x, y) (integer coordinates are pixel centres, the inverse of ndc2pix):
//   d_cam = (((2x + 1) / W - 1) tanfovx, ((2y + 1) / H - 1) tanfovy, 1)
//   d_i   = sum_j V[i][j] d_cam_j      (V = world_view_transform, row-vector convention; not normalised)
//   u = atan2(d.x, d.z) / 2pi + 0.5,  v = acos(clamp(-d.y / |d|, -1, 1)) / pi   (row 0 = world -y)
//   tx = u Ws - 0.5, ty = v Hs - 0.5, x0 = floor(tx), y0 = floor(ty); columns x0, x0 + 1 wrap modulo
//   Ws, rows y0, y0 + 1 clamp to [0, Hs - 1]; bilinear weights from fx = tx - x0, fy = ty - y0.
// The sample is evaluated as three lerps, top = t00 + fx (t01 - t00), bot likewise, top + fy (bot - top):
// a constant texture is reproduced exactly.  The backward recomputes the taps (nothing is saved by the
// forward: 12 B/pixel of ray arithmetic against 24 B/pixel of stored taps and weights) and gives
//   dL/dalpha = -sum_c g_c sky_c,   dL/dtexture[c, texel] += g_c (1 - alpha) w_texel.
//
// dL/dtexture is bitwise reproducible: the scatter adds 64-bit fixed-point integers (integer adds
// commute, whatever order the atomics arrive in), a last kernel converts the sums to fp32.
//   1. k_sky_absmax: M = max |g| over the image, an atomicMax on the float bits (order-independent).
//   2. k_sky_bwd: with e the unbiased exponent field of M (every |g| < 2^(e + 1); denormal M: e = -127)
//      and n = ceil(log2(H W)), a contribution c = g_c (1 - alpha) w is added as rint(c 2^s),
//      s = 61 - n - e.  A pixel's weights into one texel sum to at most 1 + 2^-21 (roundings of the four
//      products), so for alpha in [0, 1] a texel's sum stays below H W 2^(e + 1) (1 + 2^-21) 2^s + 4 H W / 2
//      <= 2^62 (1 + 2^-21) + 2^(n + 1) < 2^63: no overflow.  The resolution is 2^-s = 2^(n - 61) 2^e, at most
//      2^(n - 61) max|g|: 2^-40 max|g| at 1080p (n = 21), 16 bits below fp32's.  Each contribution is clamped
//      to +-2^(e + 1) before the conversion, so the conversion is always in range; sums that inputs outside
//      the contract (alpha outside [0, 1], non-finite g) push past 2^63 wrap (unsigned adds): a meaningless
//      value, in bounds and still the same on every run.
//   3. k_sky_finish: texel = (float)(sum 2^-s), written or added (fp32 old + new) to the caller's gradient.
// Neighbouring pixels share texels (at 1080p with a 2048-column texture a 16 x 16 block touches about
// 5 x 5), so a block first sums into an LDS copy of its texel bounding box (ds_add_u64) and then issues
// one global atomic per touched texel and channel.  A block whose box exceeds SKY_BOX texels -- a block
// on the atan2 seam (its unwrapped columns span the texture), next to a pole, or a texture much finer
// than the image -- adds its twelve contributions per pixel straight to global memory.
//
// dL/dviewmatrix (k_sky_bwd<true>, gs_sky_compose_backward_camera) rides on the same pass.  With
// gm_c = g_c (1 - alpha), rho^2 = d.x^2 + d.z^2, l^2 = rho^2 + d.y^2 and the sample's two slopes
//   a = sum_c gm_c [(t01 - t00) + fy ((t11 - t10) - (t01 - t00))]   (along fx)
//   b = sum_c gm_c (bot - top)                                      (along fy; 0 where the rows clamp to one)
// the ray's gradient is
//   dL/dd.x =  a (Ws / 2pi) d.z / rho^2 - b (Hs / pi) d.y d.x / (rho l^2)
//   dL/dd.z = -a (Ws / 2pi) d.x / rho^2 - b (Hs / pi) d.y d.z / (rho l^2)
//   dL/dd.y =  b (Hs / pi) rho / l^2
// and dL/dV[i][j] = sum over pixels of dL/dd_i d_cam_j (i, j < 3; floor carries no gradient, the sky at
// infinity does not see row 3 or column 3).  A pixel contributes exactly 0 when 1 - alpha == 0, when
// a == 0 and b == 0, when rho^2 == 0 or when one of its nine terms is not finite (the exact pole, a
// degenerate matrix, a non-finite g).  The nine fp32 terms of a block's pixels are summed in fp64 in a
// fixed order (through LDS, as k_camera_grad does) into one row of the scratch, and k_sky_cam_finish,
// one workgroup, adds the rows in index order: no float atomics, the same bits on every run.
#include <limits.h>

#include "gs_internal.h"

namespace gs {

constexpr int SKY_T = 16;     // pixels per block side
constexpr int SKY_MAX_BLOCKS = 512;  // blocks of the max-reduction (two per CU)
#ifndef GS_SKY_BOX
#define GS_SKY_BOX 256  // -DGS_SKY_BOX=1: no box ever fits, every block adds straight to memory (A/B builds)
#endif
constexpr int SKY_BOX = GS_SKY_BOX;  // texels of a block's LDS box (3 channels x 8 B: 6 KB)

struct SkyTap {
  int x0;          // unwrapped left column, in [-1, Ws - 1]
  int xa, xb;      // wrapped columns
  int ya, yb;      // clamped rows
  float fx, fy;
};

struct SkyRay {
  float cx, cy;      // d_cam = (cx, cy, 1)
  float dx, dy, dz;  // the world ray, not normalised
};

// Every index is forced into range whatever the ray (a degenerate view matrix gives NaN: fmaxf
// drops it), so a tap never addresses outside the texture.
__device__ __forceinline__ SkyTap sky_tap(const float* __restrict__ view, float tanfovx, float tanfovy, int W, int H,
                                          int Hs, int Ws, int x, int y, SkyRay* ray = nullptr) {
  const float cx = ((float)(2 * x + 1) / (float)W - 1.0f) * tanfovx;
  const float cy = ((float)(2 * y + 1) / (float)H - 1.0f) * tanfovy;
  const float dx = view[0] * cx + view[1] * cy + view[2];
  const float dy = view[4] * cx + view[5] * cy + view[6];
  const float dz = view[8] * cx + view[9] * cy + view[10];
  if (ray) *ray = SkyRay{cx, cy, dx, dy, dz};
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  const float u = atan2f(dx, dz) / 6.28318530717958647692f + 0.5f;
  const float v = acosf(fminf(fmaxf(-dy / len, -1.0f), 1.0f)) / 3.14159265358979323846f;
  const float tx = u * (float)Ws - 0.5f, ty = v * (float)Hs - 0.5f;
  const float x0f = floorf(tx), y0f = floorf(ty);
  SkyTap t;
  t.fx = tx - x0f;
  t.fy = ty - y0f;
  t.x0 = (int)fminf(fmaxf(x0f, -1.0f), (float)(Ws - 1));
  const int y0 = (int)fminf(fmaxf(y0f, -1.0f), (float)(Hs - 1));
  t.xa = t.x0 < 0 ? t.x0 + Ws : t.x0;
  t.xb = t.x0 + 1 >= Ws ? t.x0 + 1 - Ws : t.x0 + 1;
  t.ya = max(y0, 0);
  t.yb = min(y0 + 1, Hs - 1);
  return t;
}

__device__ __forceinline__ float sky_sample(const float* __restrict__ plane, const SkyTap& t, int Ws) {
  const float* ra = plane + (size_t)t.ya * Ws;
  const float* rb = plane + (size_t)t.yb * Ws;
  const float t00 = ra[t.xa], t01 = ra[t.xb], t10 = rb[t.xa], t11 = rb[t.xb];
  const float top = t00 + t.fx * (t01 - t00);
  const float bot = t10 + t.fx * (t11 - t10);
  return top + t.fy * (bot - top);
}

// color == nullptr: colour 0; alpha == nullptr: alpha 0 (the bare sky with both)
__global__ __launch_bounds__(SKY_T* SKY_T) void k_sky_fwd(int W, int H, const float* __restrict__ view, float tanfovx,
                                                          float tanfovy, int Hs, int Ws,
                                                          const float* __restrict__ tex,
                                                          const float* __restrict__ color,
                                                          const float* __restrict__ alpha, float* __restrict__ out) {
  const int x = blockIdx.x * SKY_T + (threadIdx.x & (SKY_T - 1));
  const int y = blockIdx.y * SKY_T + (threadIdx.x / SKY_T);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, p = (size_t)y * W + x, TS = (size_t)Hs * Ws;
  const SkyTap t = sky_tap(view, tanfovx, tanfovy, W, H, Hs, Ws, x, y);
  const float om = 1.0f - (alpha ? alpha[p] : 0.0f);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float s = sky_sample(tex + c * TS, t, Ws);
    out[c * HW + p] = (color ? color[c * HW + p] : 0.0f) + om * s;
  }
}

// zeroes the scratch (the max word and the fixed-point sums), n16 16-byte units
__global__ __launch_bounds__(256) void k_sky_clear(uint4* __restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
    dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

// max of the |g| bit patterns (sign cleared: as unsigned integers they order like the magnitudes,
// NaNs above infinity)
__global__ __launch_bounds__(256) void k_sky_absmax(const float* __restrict__ g, size_t n, uint32_t* __restrict__ maxbits) {
  uint32_t m = 0u;
  const size_t stride = (size_t)gridDim.x * 256, i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n4 = (((uintptr_t)g) & 15) == 0 ? n / 4 : 0;
  for (size_t i = i0; i < n4; i += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(g)[i];
    m = max(max(m, v.x & 0x7FFFFFFFu), max(v.y & 0x7FFFFFFFu, max(v.z & 0x7FFFFFFFu, v.w & 0x7FFFFFFFu)));
  }
  for (size_t i = 4 * n4 + i0; i < n; i += stride) m = max(m, __float_as_uint(g[i]) & 0x7FFFFFFFu);
  // one atomic per block, at most SKY_MAX_BLOCKS blocks: atomics on one word run at about 90 per
  // microsecond chip-wide (one per wave of an 8192-block grid: 280 us at 1080p; this form: 12 us)
  __shared__ uint32_t s_m[4];
  m = wave_max_u32(m);
  if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
  lds_barrier();
  if (threadIdx.x == 0) {
    m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
    if (m != 0u) atomicMax(maxbits, m);
  }
}

// the fixed-point exponent s = 61 - n - e of the header comment (n = log_hw)
__device__ __forceinline__ int sky_unbiased_exp(uint32_t maxbits) { return (int)((maxbits >> 23) & 255u) - 127; }

__device__ __forceinline__ unsigned long long sky_fixed(float c, double lim, double scale) {
  const double v = fmin(fmax((double)c, -lim), lim) * scale;  // NaN -> -lim; |v| <= 2^(62 - n)
  return (unsigned long long)(long long)__builtin_rint(v);
}

__device__ __forceinline__ bool sky_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// The pixel's nine terms of dL/dV (header comment), v[3 i + j] = dL/dd_i d_cam_j, all zero under the
// zero rules.  gc: the pixel's g, om: 1 - alpha.
__device__ __forceinline__ void sky_view_terms(const float* __restrict__ tex, size_t TS, const SkyTap& t,
                                               const SkyRay& r, int Hs, int Ws, const float gc[3], float om,
                                               float v[9]) {
  float sa[3], sb[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* ra = tex + c * TS + (size_t)t.ya * Ws;
    const float* rb = tex + c * TS + (size_t)t.yb * Ws;
    const float t00 = ra[t.xa], t01 = ra[t.xb], t10 = rb[t.xa], t11 = rb[t.xb];
    const float top = t00 + t.fx * (t01 - t00);
    const float bot = t10 + t.fx * (t11 - t10);
    sa[c] = (t01 - t00) + t.fy * ((t11 - t10) - (t01 - t00));
    sb[c] = bot - top;  // ya == yb: the same operations on the same texels, exactly 0
  }
  const float gm[3] = {gc[0] * om, gc[1] * om, gc[2] * om};
  const float a = (gm[0] * sa[0] + gm[1] * sa[1]) + gm[2] * sa[2];
  const float b = (gm[0] * sb[0] + gm[1] * sb[1]) + gm[2] * sb[2];
  const float rho2 = r.dx * r.dx + r.dz * r.dz, l2 = rho2 + r.dy * r.dy, rho = sqrtf(rho2);
  const float ak = a * ((float)Ws / 6.28318530717958647692f), bk = b * ((float)Hs / 3.14159265358979323846f);
  const float A = ak / rho2, B = bk / (rho * l2);
  const float gd[3] = {A * r.dz - (B * r.dy) * r.dx, bk * rho / l2, -(A * r.dx) - (B * r.dy) * r.dz};
  bool ok = om != 0.0f && (a != 0.0f || b != 0.0f) && rho2 != 0.0f;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    v[3 * i] = gd[i] * r.cx;
    v[3 * i + 1] = gd[i] * r.cy;
    v[3 * i + 2] = gd[i];
    ok = ok && sky_finite(v[3 * i]) && sky_finite(v[3 * i + 1]) && sky_finite(v[3 * i + 2]);
  }
  if (!ok)
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = 0.0f;
}

// dalpha == nullptr / acc == nullptr: that gradient is not produced.  maxbits: the word k_sky_absmax
// left; acc: [3, Hs, Ws] fixed-point sums (zeroed by k_sky_clear).  CAM: the block's nine sums of
// dL/dviewmatrix go to row blockIdx.y gridDim.x + blockIdx.x of cam_partial (SKY_CAM_ROW doubles).
template <bool CAM>
__global__ __launch_bounds__(SKY_T* SKY_T) void k_sky_bwd(int W, int H, const float* __restrict__ view, float tanfovx,
                                                          float tanfovy, int Hs, int Ws,
                                                          const float* __restrict__ tex,
                                                          const float* __restrict__ alpha,
                                                          const float* __restrict__ g, float* __restrict__ dalpha,
                                                          const uint32_t* __restrict__ maxbits, int log_hw,
                                                          unsigned long long* __restrict__ acc,
                                                          double* __restrict__ cam_partial) {
  __shared__ int s_box[4][4];  // per wave: min / max unwrapped column, min / max row
  __shared__ unsigned long long s_acc[3][SKY_BOX];
  const int tid = threadIdx.x;
  const int x = blockIdx.x * SKY_T + (tid & (SKY_T - 1));
  const int y = blockIdx.y * SKY_T + (tid / SKY_T);
  const bool inside = x < W && y < H;
  const size_t HW = (size_t)H * W, p = (size_t)y * W + x, TS = (size_t)Hs * Ws;
  SkyTap t = {};
  SkyRay ray = {};
  float gc[3] = {0.0f, 0.0f, 0.0f}, om = 0.0f;
  if (inside) {
    t = sky_tap(view, tanfovx, tanfovy, W, H, Hs, Ws, x, y, CAM ? &ray : nullptr);
#pragma unroll
    for (int c = 0; c < 3; c++) gc[c] = g[c * HW + p];
    om = 1.0f - (alpha ? alpha[p] : 0.0f);
    if (dalpha) {
      float s[3];
#pragma unroll
      for (int c = 0; c < 3; c++) s[c] = sky_sample(tex + c * TS, t, Ws);
      dalpha[p] = -((gc[0] * s[0] + gc[1] * s[1]) + gc[2] * s[2]);
    }
  }
  if constexpr (CAM) {
    // the block's nine sums, k_camera_grad's order: thread (k, s) adds the terms k of pixels s, s + 8,
    // ... in fp64, then the eight partial sums in order.  Lanes outside the image hold zeros.
    constexpr int STRIDE = SKY_T * SKY_T + 8;
    __shared__ float s_v[9][STRIDE];
    __shared__ double s_p[9][8];
    float v[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (inside) sky_view_terms(tex, TS, t, ray, Hs, Ws, gc, om, v);
#pragma unroll
    for (int k = 0; k < 9; k++) s_v[k][tid] = v[k];
    lds_barrier();
    if (tid < 9 * 8) {
      const float* col = &s_v[tid >> 3][tid & 7];
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < SKY_T * SKY_T / 8; k++) sum = sum + (double)col[8 * k];
      s_p[tid >> 3][tid & 7] = sum;
    }
    lds_barrier();
    if (tid < SKY_CAM_ROW) {
      double sum = 0.0;
      if (tid < 9)
#pragma unroll
        for (int s = 0; s < 8; s++) sum = sum + s_p[tid][s];
      cam_partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SKY_CAM_ROW + tid] = sum;
    }
  }
  if (!acc) return;  // uniform
  // the block's texel box: wave extents by shuffles, then the four waves' through LDS (LDS atomics of
  // 64 lanes on one word serialise: four of them per wave made this kernel 93 us at 1080p)
  for (int i = tid; i < 3 * SKY_BOX; i += SKY_T * SKY_T) (&s_acc[0][0])[i] = 0ull;
  int ext[4] = {inside ? -t.x0 : INT_MIN, inside ? t.x0 + 1 : INT_MIN, inside ? -t.ya : INT_MIN,
                inside ? t.yb : INT_MIN};  // maxima of -min / max
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
    for (int q = 0; q < 4; q++) ext[q] = max(ext[q], __shfl_xor(ext[q], d, 64));
  if (lane_id() == 0)
#pragma unroll
    for (int q = 0; q < 4; q++) s_box[tid >> 6][q] = ext[q];
  lds_barrier();
#pragma unroll
  for (int q = 0; q < 4; q++) ext[q] = max(max(s_box[0][q], s_box[1][q]), max(s_box[2][q], s_box[3][q]));
  // every block holds a pixel of the image, so the box is set; x0 >= -1 and x0 + 1 <= Ws
  const int bx0 = -ext[0], by0 = -ext[2];
  const long long bw = (long long)ext[1] - bx0 + 1, bh = (long long)ext[3] - by0 + 1;
  const bool boxed = bw * bh <= SKY_BOX;  // uniform
  const int e = sky_unbiased_exp(*maxbits);
  const double lim = __builtin_ldexp(1.0, e + 1), scale = __builtin_ldexp(1.0, 61 - log_hw - e);
  if (inside) {
    const float w[4] = {(1.0f - t.fx) * (1.0f - t.fy), t.fx * (1.0f - t.fy), (1.0f - t.fx) * t.fy, t.fx * t.fy};
    if (boxed) {
      const int ka = (t.ya - by0) * (int)bw + (t.x0 - bx0), kb = (t.yb - by0) * (int)bw + (t.x0 - bx0);
      const int k[4] = {ka, ka + 1, kb, kb + 1};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float gm = gc[c] * om;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const unsigned long long v = sky_fixed(gm * w[q], lim, scale);
          if (v) atomicAdd(&s_acc[c][k[q]], v);
        }
      }
    } else {
      const size_t o[4] = {(size_t)t.ya * Ws + t.xa, (size_t)t.ya * Ws + t.xb, (size_t)t.yb * Ws + t.xa,
                           (size_t)t.yb * Ws + t.xb};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float gm = gc[c] * om;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const unsigned long long v = sky_fixed(gm * w[q], lim, scale);
          if (v) atomicAdd(&acc[c * TS + o[q]], v);
        }
      }
    }
  }
  if (!boxed) return;
  lds_barrier();
  const int cells = (int)(bw * bh);
  for (int i = tid; i < 3 * cells; i += SKY_T * SKY_T) {
    const int c = i / cells, k = i - c * cells;
    const unsigned long long v = s_acc[c][k];
    if (v == 0ull) continue;
    const int r = k / (int)bw;
    int col = bx0 + (k - r * (int)bw);  // in [-1, Ws]
    col = col < 0 ? col + Ws : (col >= Ws ? col - Ws : col);
    atomicAdd(&acc[c * TS + (size_t)(by0 + r) * Ws + col], v);
  }
}

__global__ __launch_bounds__(256) void k_sky_finish(size_t n, const long long* __restrict__ acc,
                                                    const uint32_t* __restrict__ maxbits, int log_hw, int accumulate,
                                                    float* __restrict__ dtex) {
  const double inv = __builtin_ldexp(1.0, -(61 - log_hw - sky_unbiased_exp(*maxbits)));
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = (float)((double)acc[i] * inv);
    dtex[i] = accumulate ? dtex[i] + v : v;
  }
}

// One workgroup: the nb rows of k_sky_bwd<true> summed in fp64 in a fixed order (k_camera_grad_finish's
// form: GROUPS row groups of SKY_CAM_ROW / 2 column pairs, each thread over its rows rg, rg + GROUPS,
// ... with whole 16-B loads, then the groups in order), and the 16 floats of dL/dviewmatrix written or
// added (fp32 old + new), row 3 and column 3 as zeros.  8,160 rows (638 KB) at 1080p.
__global__ __launch_bounds__(SKY_CAM_FINISH_THREADS) void k_sky_cam_finish(const double* __restrict__ partial, long long nb,
                                                                           int accumulate, float* __restrict__ dview) {
  constexpr int PAIRS = SKY_CAM_ROW / 2, GROUPS = SKY_CAM_FINISH_THREADS / PAIRS;
  __shared__ double s_grp[GROUPS][SKY_CAM_ROW];
  __shared__ double s_fin[SKY_CAM_ROW];
  const int t = (int)threadIdx.x;
  if (t < GROUPS * PAIRS) {
    const int cp = t % PAIRS, rg = t / PAIRS;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
    for (long long r = rg; r < nb; r += GROUPS) {
      const double2 q = reinterpret_cast<const double2*>(partial)[(size_t)r * PAIRS + cp];
      a0 = a0 + q.x;
      a1 = a1 + q.y;
    }
    s_grp[rg][2 * cp] = a0;
    s_grp[rg][2 * cp + 1] = a1;
  }
  lds_barrier();
  if (t < SKY_CAM_ROW) {
    double a = 0.0;
    for (int rg = 0; rg < GROUPS; rg++) a = a + s_grp[rg][t];
    s_fin[t] = a;
  }
  lds_barrier();
  if (t < 16) {
    const float v = (t >> 2) < 3 && (t & 3) < 3 ? (float)s_fin[3 * (t >> 2) + (t & 3)] : 0.0f;
    dview[t] = accumulate ? dview[t] + v : v;
  }
}

// the view gradient's scratch: one row of SKY_CAM_ROW doubles per 16 x 16 block of the image
size_t sky_camera_scratch_bytes(int W, int H) {
  return (size_t)((W + SKY_T - 1) / SKY_T) * (size_t)((H + SKY_T - 1) / SKY_T) * SKY_CAM_ROW * sizeof(double);
}

// scratch: 16 bytes (the max word), then [3, Hs, Ws] 64-bit sums; a whole number of 16-byte units
size_t sky_scratch_bytes(int Hs, int Ws) { return (16 + 3 * (size_t)Hs * (size_t)Ws * 8 + 15) & ~(size_t)15; }

static dim3 sky_stream_grid(size_t items, size_t max_blocks = 8192) {
  const size_t nb = (items + 255) / 256;
  return dim3((unsigned)(nb < 1 ? 1 : (nb > max_blocks ? max_blocks : nb)));
}

void sky_forward(int W, int H, const float* view, float tanfovx, float tanfovy, int Hs, int Ws, const float* tex,
                 const float* color, const float* alpha, float* out, hipStream_t st) {
  const dim3 grid((W + SKY_T - 1) / SKY_T, (H + SKY_T - 1) / SKY_T);
  GS_LAUNCH("sky_fwd", k_sky_fwd, grid, dim3(SKY_T * SKY_T), 0, st, W, H, view, tanfovx, tanfovy, Hs, Ws, tex, color,
            alpha, out);
}

void sky_backward(int W, int H, const float* view, float tanfovx, float tanfovy, int Hs, int Ws, const float* tex,
                  const float* alpha, const float* dimage, float* dalpha, float* dtex, bool accumulate, char* scratch,
                  float* dview, bool accumulate_view, double* cam_scratch, hipStream_t st) {
  const dim3 grid((W + SKY_T - 1) / SKY_T, (H + SKY_T - 1) / SKY_T);
  uint32_t* maxbits = reinterpret_cast<uint32_t*>(scratch);
  unsigned long long* acc = dtex ? reinterpret_cast<unsigned long long*>(scratch + 16) : nullptr;
  const size_t n_img = 3 * (size_t)H * W, n_tex = 3 * (size_t)Hs * Ws;
  int log_hw = 0;
  while (((size_t)1 << log_hw) < (size_t)H * W) log_hw++;
  if (dtex) {
    const size_t n16 = sky_scratch_bytes(Hs, Ws) / 16;
    GS_LAUNCH("sky_clear", k_sky_clear, sky_stream_grid(n16), dim3(256), 0, st, reinterpret_cast<uint4*>(scratch), n16);
    GS_LAUNCH("sky_absmax", k_sky_absmax, sky_stream_grid(n_img / 4, SKY_MAX_BLOCKS), dim3(256), 0, st, dimage, n_img, maxbits);
  }
  if (dview)
    GS_LAUNCH("sky_bwd_cam", k_sky_bwd<true>, grid, dim3(SKY_T * SKY_T), 0, st, W, H, view, tanfovx, tanfovy, Hs, Ws,
              tex, alpha, dimage, dalpha, maxbits, log_hw, acc, cam_scratch);
  else
    GS_LAUNCH("sky_bwd", k_sky_bwd<false>, grid, dim3(SKY_T * SKY_T), 0, st, W, H, view, tanfovx, tanfovy, Hs, Ws,
              tex, alpha, dimage, dalpha, maxbits, log_hw, acc, (double*)nullptr);
  if (dview)
    GS_LAUNCH("sky_cam_finish", k_sky_cam_finish, dim3(1), dim3(SKY_CAM_FINISH_THREADS), 0, st, cam_scratch,
              (long long)grid.x * grid.y, accumulate_view ? 1 : 0, dview);
  if (dtex)
    GS_LAUNCH("sky_finish", k_sky_finish, sky_stream_grid(n_tex), dim3(256), 0, st, n_tex,
              reinterpret_cast<const long long*>(acc), maxbits, log_hw, accumulate ? 1 : 0, dtex);
}

}  // namespace gs
