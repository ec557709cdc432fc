#include <dlfcn.h>

#include <atomic>
#include <cstdlib>
// gs_api.hip -- C ABI (include/gsrast.h): argument validation, buffer layout, stage orchestration,
// error capture, debug synchronisation and per-kernel HIP-event timing.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/gsrast.h"
#include "gs_internal.h"

namespace gs {

// ------------------------------------------------------------------------------------------
// error / debug / timing state
// ------------------------------------------------------------------------------------------
static thread_local std::string t_err;
static thread_local bool t_failed = false;
static thread_local bool t_debug = false;

static void set_error(const char* fmt, ...) {
  if (t_failed) return;  // keep the first error
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  t_err = buf;
  t_failed = true;
}
static void clear_error(int debug) {
  t_err.clear();
  t_failed = false;
  t_debug = debug != 0;
}

struct ProfEntry {
  std::string name;
  double ms;
  long long n;
};
struct Pending {
  const char* name;
  hipEvent_t a, b;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<Pending> g_pending;
static std::vector<hipEvent_t> g_pool;
static std::vector<ProfEntry> g_stats;

static hipEvent_t get_event() {
  if (!g_pool.empty()) {
    hipEvent_t e = g_pool.back();
    g_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void trace_begin(const char* name, hipStream_t st) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  hipEvent_t a = get_event();
  (void)hipEventRecord(a, st);
  g_pending.push_back(Pending{name, a, nullptr});
}

void trace_end(const char* name, hipStream_t st) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) set_error("kernel %s launch failed: %s", name, hipGetErrorString(e));
  if (g_prof_on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t b = get_event();
    (void)hipEventRecord(b, st);
    if (!g_pending.empty() && g_pending.back().b == nullptr) g_pending.back().b = b;
  }
  if (t_debug) {
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) set_error("kernel %s failed: %s", name, hipGetErrorString(e));
  }
}

static std::atomic<int> g_launch_log{-1};  // -1: not yet read from GSRAST_LAUNCH_LOG
static std::mutex g_launch_mu;
static std::vector<const void*> g_launched;

static int launch_log_on() {
  int v = g_launch_log.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("GSRAST_LAUNCH_LOG");
    v = (e && atoi(e) != 0) ? 1 : 0;
    g_launch_log.store(v, std::memory_order_relaxed);
  }
  return v;
}

void launch_record(const void* k) {
  if (!launch_log_on()) return;
  std::lock_guard<std::mutex> lk(g_launch_mu);
  for (const void* x : g_launched)
    if (x == k) return;
  g_launched.push_back(k);
}

void host_error(const char* msg) { set_error("%s", msg); }

static bool check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) set_error("%s failed: %s", what, hipGetErrorString(e));
  return e == hipSuccess;
}

static CameraArgs make_camera(const float* bg, int W, int H, const float* view, const float* proj, const float* campos,
                              float tanfovx, float tanfovy, int prefiltered) {
  CameraArgs c;
  c.view = view;
  c.proj = proj;
  c.campos = campos;
  c.bg = bg;
  c.tanfovx = tanfovx;
  c.tanfovy = tanfovy;
  c.fy = (float)H / (2.0f * tanfovy);
  c.fx = (float)W / (2.0f * tanfovx);
  c.W = W;
  c.H = H;
  // (64-bit: a size the checks below refuse must not overflow on the way to them)
  c.gx = (int)(((long long)W + GS_TILE - 1) / GS_TILE);
  c.gy = (int)(((long long)H + GS_TILE - 1) / GS_TILE);
  c.prefiltered = prefiltered;
  return c;
}

// a camera that carries an image size only (the buffer layouts and the binning read nothing else)
static CameraArgs size_camera(int W, int H) {
  return make_camera(nullptr, W, H, nullptr, nullptr, nullptr, 1.0f, 1.0f, 0);
}

// The image-size limits of include/gsrast.h, for a positive size.  GS_MAX_GRID_DIM: preprocess_view
// packs a Gaussian's tile rectangle as x0 | x1 << 16, y0 | y1 << 16 with x1 <= gx, y1 <= gy (binrec,
// read back by span_of).  GS_MAX_TILES: tile_finish keeps bucket << 22 | rank per tile (tile_brank),
// k_tile_order reads the rank with & 0x3FFFFF, and a rank is below the tile count.  Within these the
// int products gx * gy, the uint32 sched_words(tiles) = 2 tiles + 513, the render grid of
// xcd_span(tiles) * 32 workgroups and tile_bits(tiles) <= 22 (three tile-sort passes) all hold; pixel
// indices are size_t.
static bool size_within_limits(int W, int H) {
  const long long gx = ((long long)W + GS_TILE - 1) / GS_TILE, gy = ((long long)H + GS_TILE - 1) / GS_TILE;
  return gx <= GS_MAX_GRID_DIM && gy <= GS_MAX_GRID_DIM && gx * gy <= (long long)GS_MAX_TILES;
}
#define GS_E_SIZE_LIMIT \
  "image size %d x %d is too large: at most 65535 tiles of 16 pixels per row and per column and 4194304 tiles in all"
// the check itself, behind each entry's positive-size check (the text after an entry's own prefix)
static bool size_limit_error(int W, int H, const char* prefix = "") {
  if (size_within_limits(W, H)) return false;
  char fmt[256];
  snprintf(fmt, sizeof(fmt), "%s%s", prefix, GS_E_SIZE_LIMIT);
  set_error(fmt, W, H);
  return true;
}
// the sizing queries: 0 bytes for such a size, the message left without failing the thread's next call
static bool size_query_refused(int W, int H) {
  if (W <= 0 || H <= 0 || size_within_limits(W, H)) return false;
  char buf[256];
  snprintf(buf, sizeof(buf), GS_E_SIZE_LIMIT, W, H);
  t_err = buf;
  return true;
}

// The scene of a call, packed once at the ABI boundary, in the entries' own argument order
// (shs_rest: the split SH rows, null in the entries without them).
static GaussianArgs make_scene(int P, int D, int M, const float* means3D, const float* shs, const float* shs_rest,
                               const float* colors, const float* opacities, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D) {
  return GaussianArgs{P, D, M, means3D, shs, colors, opacities, scales, rotations, cov3D, scale_modifier, shs_rest};
}

// The scene and camera checks of every forward / backward entry.  Their order is part of the
// contract (which of two faults is reported; tests/test_api_contract_cpu.py pins it).
static bool validate(const GaussianArgs& g, const CameraArgs& c, bool need_opac = true) {
  if (g.P < 0) return set_error("P must be >= 0"), false;
  if (c.W <= 0 || c.H <= 0) return set_error("image size must be positive (got %d x %d)", c.W, c.H), false;
  if (size_limit_error(c.W, c.H)) return false;
  if (g.P > 0) {
    if (!g.means3D || (need_opac && !g.opacities) || !c.view || !c.proj || !c.bg)
      return set_error("missing required input pointer"), false;
    if ((g.shs == nullptr) == (g.colors == nullptr))
      return set_error("Please provide excatly one of either SHs or precomputed colors!"), false;
    if (((g.scales == nullptr || g.rotations == nullptr) && g.cov3D == nullptr) ||
        ((g.scales || g.rotations) && g.cov3D))
      return set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"), false;
    if (g.shs) {
      if (g.D < 0 || g.D > 3) return set_error("SH degree must be in [0, 3] (got %d)", g.D), false;
      if (g.M < (g.D + 1) * (g.D + 1))
        return set_error("shs has %d coefficients, degree %d needs %d", g.M, g.D, (g.D + 1) * (g.D + 1)), false;
      if (!c.campos) return set_error("campos is required with SHs"), false;
    }
    if ((size_t)g.P * 48 > ((size_t)1 << 40)) return set_error("P too large"), false;
  }
  // split SH inputs (features_dc + features_rest rows; also checked for an empty scene): shs_rest
  // needs SH colours with M >= 2
  if (!g.shs_rest) return true;
  if (!g.shs || g.colors) return set_error("split SH: features_dc and features_rest replace shs (no colours)"), false;
  if (g.M < 2) return set_error("split SH: M must be >= 2 (got %d)", g.M), false;
  return true;
}

// The three buffers of a view laid out: P Gaussians, I instances, the camera's image size
// (a null base pointer leaves that part unset).
struct Layouts {
  GeomPtrs geo;
  BinPtrs bin;
  ImgPtrs img;
  Layouts(int P, long long I, const CameraArgs& c, const void* geom, const void* binning, const void* image) {
    geom_layout((size_t)P, &geo, (char*)geom);
    bin_layout((size_t)I, c.gx * c.gy, &bin, (char*)binning);
    img_layout(c.W, c.H, &img, (char*)image);
  }
};

// ------------------------------------------------------------------------------------------
// debug export kernel
// ------------------------------------------------------------------------------------------
// entries past the list's device count (past a bounded buffer's capacity) are not written by the
// forward: exported as ~0 (no gather through them)
__global__ void k_export_list(uint32_t I, const uint32_t* counters, const uint32_t* point_list, const uint32_t* ids,
                              uint32_t* out) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= I) return;
  const uint32_t n = min(I, counters[CNT_I]);
  if (k >= n) {
    out[k] = 0xFFFFFFFFu;
    return;
  }
  const uint32_t s = point_list[k];
  out[k] = s < I ? ids[s] : 0xFFFFFFFFu;
}
__global__ void k_export_splat(int P, const float4* splat, float* xy, float* co, float* rgb, float* depth) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float4 a = splat[3 * i], b = splat[3 * i + 1], d = splat[3 * i + 2];
  if (xy) {
    xy[2 * i] = a.x;
    xy[2 * i + 1] = a.y;
  }
  if (co) {
    co[4 * i] = a.z;
    co[4 * i + 1] = a.w;
    co[4 * i + 2] = b.x;
    co[4 * i + 3] = b.y;
  }
  if (rgb) {
    rgb[3 * i] = b.z;
    rgb[3 * i + 1] = b.w;
    rgb[3 * i + 2] = d.x;
  }
  if (depth) depth[i] = d.y;
}

}  // namespace gs

using namespace gs;

namespace gs {
static std::atomic<int> g_exact_exp{-1};  // -1: not yet read from GSRAST_EXACT_EXP
bool exact_exp() {
  int v = g_exact_exp.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("GSRAST_EXACT_EXP");
    v = (e && e[0] && e[0] != '0') ? 1 : 0;
    g_exact_exp.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}
}  // namespace gs

namespace gs {
static std::atomic<uint32_t> g_spin_limit{LB_SPIN_LIMIT};
uint32_t scan_spin_limit() { return g_spin_limit.load(std::memory_order_relaxed); }
static std::atomic<int> g_tile_sort_packed{1};
static std::atomic<long long> g_tile_sort_packed_n{0};
bool tile_sort_packed() { return g_tile_sort_packed.load(std::memory_order_relaxed) != 0; }
void tile_sort_packed_note() { g_tile_sort_packed_n.fetch_add(1, std::memory_order_relaxed); }

// row waits installed by gs_set_row_waits, per host thread, until the next forward preprocess
static thread_local RowWait t_row_waits[GS_MAX_ROW_WAITS];
static thread_local int t_row_wait_count = 0;
int take_row_waits(RowWait* out, int max) {
  const int n = t_row_wait_count < max ? t_row_wait_count : max;
  for (int k = 0; k < n; k++) out[k] = t_row_waits[k];
  t_row_wait_count = 0;
  return n;
}
bool stream_wait(hipStream_t st, hipEvent_t ev) {
  const hipError_t e = hipStreamWaitEvent(st, ev, 0);
  if (e != hipSuccess) set_error("row wait: hipStreamWaitEvent failed: %s", hipGetErrorString(e));
  return e == hipSuccess;
}
uint32_t next_scan_epoch() {
  static std::atomic<uint32_t> e{0};
  return (e.fetch_add(1, std::memory_order_relaxed) % ((1u << 30) - 1u)) + 1u;
}
}  // namespace gs

extern "C" {

int gs_abi_version(void) { return GSRAST_ABI_VERSION; }
const char* gs_last_error(void) { return t_err.c_str(); }

size_t gs_geom_buffer_bytes(int P) { return geom_layout((size_t)(P > 0 ? P : 1), nullptr, nullptr); }
size_t gs_binning_buffer_bytes(long long num_rendered, int W, int H) {
  if (size_query_refused(W, H)) return 0;
  int tiles = ((W + GS_TILE - 1) / GS_TILE) * ((H + GS_TILE - 1) / GS_TILE);
  return bin_layout((size_t)(num_rendered > 0 ? num_rendered : 1), tiles, nullptr, nullptr);
}
size_t gs_image_buffer_bytes(int W, int H) {
  if (size_query_refused(W, H)) return 0;
  return img_layout(W, H, nullptr, nullptr);
}
long long gs_binning_layout_count(size_t bytes, int W, int H) {
  // every array of bin_layout has a size that never decreases with the count (sort_scratch_words
  // is a monotone bound, not sort_plan's nb), so gs_binning_buffer_bytes is non-decreasing, and two
  // counts with the same byte size have the same aligned array sizes, hence the same layout: the
  // largest count that fits `bytes` lays the buffer out exactly as the count it was sized for
  // (tests/test_abi.py checks this around the sort's block-count steps at k * 2^23 instances)
  if (size_query_refused(W, H)) return 0;
  if (gs_binning_buffer_bytes(1, W, H) > bytes) return 0;
  long long lo = 1, hi = GS_MAX_INSTANCES;
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (gs_binning_buffer_bytes(mid, W, H) <= bytes)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}
size_t gs_grad_buffer_bytes(long long num_rendered) {
  const size_t R = (size_t)(num_rendered > 0 ? num_rendered : 1);
  return align_up(R * GRAD_REC * sizeof(float));
}
size_t gs_grad_buffer_bytes_aux(long long num_rendered, int P) {
  return grad_layout_aux((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)(P > 0 ? P : 1), nullptr, nullptr);
}
size_t gs_grad_buffer_bytes_absgrad(long long num_rendered, int P) {
  return grad_layout_abs((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)(P > 0 ? P : 1), nullptr, nullptr);
}

// Pinned, device-mapped host words: kernels store into them directly (vector stores through the
// device pointer), so a readback costs no copy launch.
static bool mapped_words(size_t bytes, uint32_t** host, uint32_t** dev) {
  void* p = nullptr;
  void* d = nullptr;
  if (!check_hip(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc")) return false;
  if (!check_hip(hipHostGetDevicePointer(&d, p, 0), "hipHostGetDevicePointer")) return false;
  memset(p, 0, bytes);
  *host = (uint32_t*)p;
  *dev = (uint32_t*)d;
  return true;
}

// Per-thread, per-device readback words + events (reused call after call: a call waits on its
// events before returning, so the slot is free again when the next call starts).  View v's
// totals land in words [8 v, 8 v + 4): instances low / high, V, error flags (CounterFinalize).
struct ReadbackSlot {
  uint32_t* host = nullptr;
  uint32_t* dev = nullptr;
  hipEvent_t ev[FUSED_MAX_VIEWS] = {};  // view v's totals written (the first depth-sort histogram launch)
};
static ReadbackSlot* readback_slot() {
  static thread_local ReadbackSlot slots[64];
  int dev = 0;
  if (!check_hip(hipGetDevice(&dev), "hipGetDevice")) return nullptr;
  if (dev < 0 || dev >= 64) return set_error("device ordinal out of range"), nullptr;
  ReadbackSlot& s = slots[dev];
  if (!s.host) {
    if (!mapped_words(32 * FUSED_MAX_VIEWS, &s.host, &s.dev)) return nullptr;
    for (int v = 0; v < FUSED_MAX_VIEWS; v++)
      if (!check_hip(hipEventCreateWithFlags(&s.ev[v], hipEventDisableTiming), "hipEventCreate")) return nullptr;
  }
  return &s;
}

// view v's instance count from its readback words; false (error set) for an invalid view
static bool read_view_totals(const uint32_t* w, int v, int views, long long* num_rendered) {
  const uint32_t err = w[3];
  const unsigned long long I = (unsigned long long)w[1] << 32 | w[0];
  if (err & ERR_PREFILTERED) return set_error("Point is filtered although prefiltered is set. This shouldn't happen!"), false;
  if ((err & ERR_INSTANCES) || I > (unsigned long long)GS_MAX_INSTANCES) {
    if (views > 1) return set_error("view %d has %llu (Gaussian, tile) instances, more than %lld", v, I, GS_MAX_INSTANCES), false;
    return set_error("the view has %llu (Gaussian, tile) instances, more than %lld", I, GS_MAX_INSTANCES), false;
  }
  *num_rendered = (long long)I;
  return true;
}

// Error flags of the last forwards' sorts / scans, per device (not per thread: the backward of a
// forward runs on the autograd engine's device thread).  Each gs_forward_render's render kernel
// stores them into a pinned word of a small ring, behind an event; once its own launches are
// queued, a forward checks the forwards queued before it, and the next backward or forward call
// checks this one (ERR_LOOKBACK: a look-back wait ran out), so no host wait idles the GPU.
// A forward reserves its word and its sequence number in one critical section; reusing a word
// first checks the forward that last held it, so concurrent host threads never share or drop one.
constexpr int ORDER_RING = 8;
struct OrderFlags {
  std::mutex mu;
  uint32_t* host = nullptr;  // words 16 k (k < ORDER_RING): the ordering error flags of forward seq % ORDER_RING
  uint32_t* dev = nullptr;   // device pointer of `host`
  hipEvent_t ev[ORDER_RING] = {};
  int state[ORDER_RING] = {};  // 0 free, 1 reserved (render not queued yet), 2 queued, not checked
  unsigned long long seq = 0;  // forwards that reserved a word so far
};
static OrderFlags g_order[64];

static OrderFlags* order_flags() {
  int dev = 0;
  if (!check_hip(hipGetDevice(&dev), "hipGetDevice")) return nullptr;
  if (dev < 0 || dev >= 64) return set_error("device ordinal out of range"), nullptr;
  return &g_order[dev];
}

// check ring slot k's queued forward (waits for its render kernel; with wait=false a forward whose
// render has not finished yet stays queued for a later check); true: failed (error set)
static bool check_order_slot_locked(OrderFlags& o, int k, bool wait = true) {
  if (o.state[k] != 2) return false;
  if (!wait) {
    const hipError_t q = hipEventQuery(o.ev[k]);
    if (q == hipErrorNotReady) return false;
    if (!check_hip(q, "hipEventQuery")) return true;
  }
  o.state[k] = 0;
  if (!check_hip(hipEventSynchronize(o.ev[k]), "hipEventSynchronize")) return true;
  if (o.host[16 * k] & ERR_LOOKBACK) {
    set_error("forward ordering: a look-back wait of the offsets scan or a one-sweep sort timed out "
              "(the instance list of that forward is invalid)");
    return true;
  }
  return false;
}
// every queued forward's flags.  wait=false (the backward entry points): only the forwards whose
// render kernel has finished -- a backward is queued right behind its forward's render, and waiting
// for that render here would stall the host while the device has work; a forward whose render
// has not finished is checked by the next call (at the latest the next forward, whose instance-count
// readback comes after it on the stream)
// skip: a forward (sequence number) left out, e.g. the caller's own, whose render was just queued
static bool check_order_flags(bool wait = true, long long skip = -1) {
  OrderFlags* o = order_flags();
  if (!o) return true;
  std::lock_guard<std::mutex> lk(o->mu);
  bool failed = false;
  for (int k = 0; k < ORDER_RING; k++)
    if (skip < 0 || k != (int)(skip % ORDER_RING)) failed |= check_order_slot_locked(*o, k, wait);
  return failed;
}

// forward q's flags now (waits for its render kernel), if its word still holds them; true: failed
static bool check_order_seq(unsigned long long q) {
  OrderFlags* o = order_flags();
  if (!o) return true;
  std::lock_guard<std::mutex> lk(o->mu);
  const int k = (int)(q % ORDER_RING);
  return o->seq - q <= (unsigned long long)ORDER_RING && check_order_slot_locked(*o, k);
}

// The device word this forward's render kernel stores its ordering flags into, and (*seq_out) the
// forward's sequence number; null on error.
static uint32_t* order_flags_word(unsigned long long* seq_out) {
  OrderFlags* o = order_flags();
  if (!o) return nullptr;
  std::lock_guard<std::mutex> lk(o->mu);
  if (!o->host) {
    if (!mapped_words(16 * ORDER_RING, &o->host, &o->dev)) return nullptr;
    for (int k = 0; k < ORDER_RING; k++)
      if (!check_hip(hipEventCreateWithFlags(&o->ev[k], hipEventDisableTiming), "hipEventCreate")) return nullptr;
  }
  const unsigned long long q = o->seq;
  const int k = (int)(q % ORDER_RING);
  if (o->state[k] == 1) return set_error("more than %d forwards queueing at once on one device", ORDER_RING), nullptr;
  if (check_order_slot_locked(*o, k)) return nullptr;  // the word's previous forward
  o->seq++;
  o->state[k] = 1;
  *seq_out = q;
  // the render stores nonzero flags only: clear the word
  o->host[16 * k] = 0u;
  return o->dev + 16 * k;
}
// the render kernel that stores forward `q`'s flags is queued on `st`: record its event, then
// check the forwards queued before it whose renders have finished (no wait: the views of a step
// render on two streams, and waiting here for the previous view's render stalled the host for that
// render's length in every step; the unfinished ones are checked after the next count readback)
static bool queue_order_flags(hipStream_t st, unsigned long long q) {
  OrderFlags* o = order_flags();
  if (!o) return true;
  std::lock_guard<std::mutex> lk(o->mu);
  const int k = (int)(q % ORDER_RING);
  if (!check_hip(hipEventRecord(o->ev[k], st), "hipEventRecord")) {
    o->state[k] = 0;
    return true;
  }
  o->state[k] = 2;
  bool failed = false;
  for (int j = 0; j < ORDER_RING; j++)
    if (j != k) failed |= check_order_slot_locked(*o, j, false);
  return failed;
}
// a forward that reserved a word and failed before queueing its render gives the word back
static void release_order_word(unsigned long long q) {
  OrderFlags* o = order_flags();
  if (!o) return;
  std::lock_guard<std::mutex> lk(o->mu);
  const int k = (int)(q % ORDER_RING);
  if (o->state[k] == 1) o->state[k] = 0;
}

// Status of bounded forwards (gs_forward_bounded), per device: pinned words the kernels store into
// only when a view has error flags -- [0] the preprocess totals' flags (CounterFinalize) with [1], [2]
// that view's instance count, [4] the ordering flags (render kernel) -- so no event, no host wait
// and nothing per call (HIP-graph capturable).  gs_bounded_status reads and clears them.
struct BoundedStatus {
  std::mutex mu;
  uint32_t* host = nullptr;
  uint32_t* dev = nullptr;
};
static BoundedStatus g_bounded[64];
static BoundedStatus* bounded_status() {
  int dev = 0;
  if (!check_hip(hipGetDevice(&dev), "hipGetDevice")) return nullptr;
  if (dev < 0 || dev >= 64) return set_error("device ordinal out of range"), nullptr;
  BoundedStatus& b = g_bounded[dev];
  std::lock_guard<std::mutex> lk(b.mu);
  if (!b.host && !mapped_words(64, &b.host, &b.dev)) return nullptr;
  return &b;
}
// flags of the bounded forwards since the last read (0: none), and the instance count of a view that
// raised them; clears them
static uint32_t take_bounded_status(BoundedStatus* b, long long* instances) {
  std::lock_guard<std::mutex> lk(b->mu);
  uint32_t* w = b->host;
  // take and clear each flag word in one atomic exchange: a bounded kernel still in flight that
  // stores its flags between a read and a clear would otherwise lose them (the count words are
  // only meaningful beside a flag, so they are taken after the flags)
  const uint32_t f = __atomic_exchange_n(&w[0], 0u, __ATOMIC_ACQ_REL) | __atomic_exchange_n(&w[4], 0u, __ATOMIC_ACQ_REL);
  const uint32_t lo = __atomic_exchange_n(&w[1], 0u, __ATOMIC_ACQ_REL), hi = __atomic_exchange_n(&w[2], 0u, __ATOMIC_ACQ_REL);
  if (instances) *instances = f ? (long long)((unsigned long long)hi << 32 | lo) : 0;
  return f;
}
static bool bounded_status_error(uint32_t f, long long inst) {
  if (f & ERR_PREFILTERED) return set_error("Point is filtered although prefiltered is set. This shouldn't happen!"), true;
  if (f & (ERR_CAPACITY | ERR_INSTANCES))
    return set_error("bounded forward: a view had %lld (Gaussian, tile) instances, more than its binning capacity "
                     "(its image and gradients are invalid; rerun with a larger capacity)", inst), true;
  if (f & ERR_LOOKBACK)
    return set_error("bounded forward: a look-back wait of the offsets scan or a one-sweep sort timed out "
                     "(the instance list of that forward is invalid)"), true;
  return false;
}

// the status words for a new bounded forward, once an earlier one's flags are reported; null: error set
static BoundedStatus* bounded_status_checked() {
  BoundedStatus* bs = bounded_status();
  long long inst = 0;
  return bs && !bounded_status_error(take_bounded_status(bs, &inst), inst) ? bs : nullptr;
}

// ---- forward: each entry packs its arguments once (make_scene, make_camera, FwdOut) and runs shared steps ----
// What a single-view forward writes (the preprocess entries: radii and geom only)
struct FwdOut {
  int* radii;  // written by the preprocess, read by the binning
  void* geom;
  long long num_rendered;  // the instance count the binning buffer is laid out for (bounded / counted: the capacity)
  void* binning;
  void* image;
  float* out_color;
  FwdAux aux;
};

// The render tail: the binning (TAIL_BIN) and the compositing of a view whose ordering is queued.
// TAIL_BOUNDED: the ordering's error flags go to the sticky bounded-status word, nothing is
// recorded or checked here.  The caller has checked the arguments.
enum : unsigned { TAIL_BIN = 1u, TAIL_BOUNDED = 2u };
static int render_tail(int P, const CameraArgs& c, const FwdOut& o, unsigned mode, hipStream_t st,
                       unsigned long long* oseq_out = nullptr) {
  const bool bounded = (mode & TAIL_BOUNDED) != 0;
  const Layouts L(P, o.num_rendered, c, o.geom, o.binning, o.image);
  // the look-back waits of the offsets scan and of the one-sweep sorts (never expected to run out:
  // the waited-for workgroups are running) leave ERR_LOOKBACK; the render kernel stores the flags
  // into pinned memory, behind an event that the next backward or forward call checks, so no host
  // wait idles the device
  BoundedStatus* bs = bounded ? bounded_status() : nullptr;
  unsigned long long oseq = 0;
  uint32_t* flags_word = bounded ? (bs ? bs->dev + 4 : nullptr) : order_flags_word(&oseq);
  if (!flags_word) return 1;
  if (mode & TAIL_BIN) fwd_bin(P, (uint32_t)o.num_rendered, c, o.radii, L.geo, L.bin, L.img, st);
  fwd_render(c, L.geo, L.bin, L.img, o.out_color, st, flags_word, o.aux);
  if (!bounded) {
    if (oseq_out) *oseq_out = oseq;
    if (t_failed) release_order_word(oseq);
    else if (queue_order_flags(st, oseq)) return 1;
  }
  return t_failed ? 1 : 0;
}

// Where a single-view forward's instance totals go: read back before the binning buffer is sized
// (gs_forward_preprocess: the call ends behind the ordering), into the sticky bounded-status words
// (gs_forward_bounded: no host wait), or read back at the end of a whole forward that is queued
// against a capacity meanwhile (gs_forward_counted).
enum class Totals { ReadBack, Bounded, Counted };
// The single-view forward: validation, the preprocess and the ordering, then what `mode` asks for.
// The order of the checks and of their side effects is part of the contract.
// aa (gs_forward_preprocess_aa): the antialiased preprocess kernels; nothing else differs.
static int forward_view(const GaussianArgs& g, const CameraArgs& c, const FwdOut& o, Totals mode,
                        long long* num_rendered_host, int debug, hipStream_t st, bool aa = false) {
  const int P = g.P;
  const bool whole = mode != Totals::ReadBack;  // the binning and the render follow in this call
  clear_error(debug);
  if (mode != Totals::Bounded && num_rendered_host) *num_rendered_host = 0;
  if (!validate(g, c)) return 1;
  if (P == 0) return 0;
  if (whole && (o.num_rendered < 0 || o.num_rendered > GS_MAX_INSTANCES)) return set_error("capacity out of range"), 1;
  if (!o.radii || !o.geom || (mode != Totals::Bounded && !num_rendered_host) ||
      (whole && (!o.binning || !o.image || !o.out_color)))
    return set_error(whole ? "missing buffer pointer" : "missing output pointer"), 1;
  BoundedStatus* bs = nullptr;
  ReadbackSlot* rb = nullptr;
  if (mode == Totals::Bounded) {
    if (!(bs = bounded_status_checked())) return 1;
  } else {
    // num_rendered is the sum of the per-Gaussian tile counts, known when the first depth-sort
    // histogram launch has summed the preprocess workgroups' totals: that launch stores it straight
    // into pinned memory, and the host waits for it while the GPU goes on with the depth sort and
    // the instance offsets (Counted: the binning and the render too), so the round trip overlaps device work.
    if (!(rb = readback_slot())) return 1;
    // earlier forwards' look-back waits: the finished ones now (no wait before the launches), then,
    // after this forward's own readback (behind them on the stream), the rest
    if (check_order_flags(false)) return 1;
  }
  GeomPtrs geo;
  geom_layout((size_t)P, &geo, (char*)o.geom);
  fwd_preprocess(g, c, o.radii, geo, st, aa);
  const uint32_t cap32 = (uint32_t)o.num_rendered;
  fwd_order(P, geo, st, rb ? rb->dev : nullptr, rb ? rb->ev[0] : nullptr, whole ? &cap32 : nullptr,
            bs ? bs->dev : nullptr);
  if (mode == Totals::Bounded) return t_failed ? 1 : render_tail(P, c, o, TAIL_BIN | TAIL_BOUNDED, st);
  // the count readback is queued into this thread's slot: every return from here on waits for it,
  // so no kernel of this call can still write the slot's words when the thread's next call reads them
  auto drain = [&]() { (void)hipEventSynchronize(rb->ev[0]); };
  if (t_failed) return drain(), 1;
  unsigned long long oseq = 0;
  if (whole && render_tail(P, c, o, TAIL_BIN, st, &oseq)) return drain(), 1;
  if (!check_hip(hipEventSynchronize(rb->ev[0]), "hipEventSynchronize")) return 1;
  // the rest of the earlier forwards (Counted: but this one, whose render was just queued)
  if (check_order_flags(true, whole ? (long long)oseq : -1)) return 1;
  long long I = 0;
  if (!read_view_totals(rb->host, 0, 1, &I)) return 1;
  *num_rendered_host = I;
  if (whole && I > o.num_rendered) {
    // the queued binning and render skipped their work (ERR_CAPACITY): clear the flag so that
    // gs_forward_render can bin the same geometry into a buffer of the exact size
    fwd_clear_flags(geo, ERR_CAPACITY, st);
    // the skipped render carries this ordering's look-back flags: read them now (it finishes
    // quickly, having skipped its work), so a timed-out ordering fails here, once, instead of
    // again at the next call through the re-binned forward's flags
    if (t_failed || check_order_seq(oseq)) return 1;
    return GS_COUNT_SHORT;
  }
  return 0;
}

int gs_forward_preprocess(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                          const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                          float tan_fovy, int prefiltered, int* radii_out, void* geom_buffer,
                          long long* num_rendered_host, int debug, void* stream) {
  return forward_view(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, prefiltered),
      FwdOut{radii_out, geom_buffer}, Totals::ReadBack, num_rendered_host, debug, (hipStream_t)stream);
}

int gs_forward_preprocess_aa(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                             const float* shs, const float* colors_precomp, const float* opacities,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                             const float* campos, float tan_fovx, float tan_fovy, int prefiltered, int* radii_out,
                             void* geom_buffer, long long* num_rendered_host, int debug, void* stream,
                             int antialiasing) {
  return forward_view(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, prefiltered),
      FwdOut{radii_out, geom_buffer}, Totals::ReadBack, num_rendered_host, debug, (hipStream_t)stream,
      antialiasing != 0);
}

int gs_forward_preprocess_split(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                                const float* shs_dc, const float* shs_rest, const float* opacities,
                                const float* scales, float scale_modifier, const float* rotations,
                                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                const float* campos, float tan_fovx, float tan_fovy, int prefiltered, int* radii_out,
                                void* geom_buffer, long long* num_rendered_host, int debug, void* stream) {
  if (!shs_rest) {
    clear_error(debug);
    if (num_rendered_host) *num_rendered_host = 0;
    return set_error("split SH: features_rest is NULL"), 1;
  }
  return forward_view(
      make_scene(P, D, M, means3D, shs_dc, shs_rest, nullptr, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, prefiltered),
      FwdOut{radii_out, geom_buffer}, Totals::ReadBack, num_rendered_host, debug, (hipStream_t)stream);
}

// gs_forward_render and its variants: the tail behind its own checks (only the binning needs radii)
static int forward_render(int P, const CameraArgs& c, const FwdOut& o, unsigned mode, int debug, hipStream_t st) {
  clear_error(debug);
  if (P <= 0) return 0;
  if (c.W <= 0 || c.H <= 0) return set_error("image size must be positive"), 1;
  if (size_limit_error(c.W, c.H)) return 1;
  if (o.num_rendered < 0 || o.num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
  if (!o.geom || !o.binning || !o.image || !o.out_color || ((mode & TAIL_BIN) && !o.radii))
    return set_error("missing buffer pointer"), 1;
  return render_tail(P, c, o, mode, st);
}
// (the render reads the radii; FwdOut carries them as the preprocess writes them)
static FwdOut render_out(const int* radii, void* geom, long long num_rendered, void* binning, void* image,
                         float* out_color, float* invdepth = nullptr, float* alpha = nullptr) {
  return FwdOut{const_cast<int*>(radii), geom, num_rendered, binning, image, out_color, FwdAux{invdepth, alpha}};
}

int gs_forward_render(int P, const float* background, int W, int H, const float* viewmatrix, const float* projmatrix,
                      const float* campos, float tan_fovx, float tan_fovy, const int* radii, void* geom_buffer,
                      long long num_rendered, void* binning_buffer, void* image_buffer, float* out_color, int debug,
                      void* stream) {
  return forward_render(P, make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0),
                        render_out(radii, geom_buffer, num_rendered, binning_buffer, image_buffer, out_color),
                        TAIL_BIN, debug, (hipStream_t)stream);
}

int gs_forward_render_aux(int P, const float* background, int W, int H, const float* viewmatrix,
                          const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                          const int* radii, void* geom_buffer, long long num_rendered, void* binning_buffer,
                          void* image_buffer, float* out_color, float* out_invdepth, float* out_alpha, int debug,
                          void* stream) {
  return forward_render(P, make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0),
                        render_out(radii, geom_buffer, num_rendered, binning_buffer, image_buffer, out_color,
                                   out_invdepth, out_alpha),
                        TAIL_BIN, debug, (hipStream_t)stream);
}

int gs_forward_render_bounded(int P, const float* background, int W, int H, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                              const int* radii, void* geom_buffer, long long capacity, void* binning_buffer,
                              void* image_buffer, float* out_color, int debug, void* stream) {
  return forward_render(P, make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0),
                        render_out(radii, geom_buffer, capacity, binning_buffer, image_buffer, out_color),
                        TAIL_BIN | TAIL_BOUNDED, debug, (hipStream_t)stream);
}

int gs_forward_render_binned(int P, const float* background, int W, int H, const float* viewmatrix,
                             const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                             void* geom_buffer, long long num_rendered, void* binning_buffer, void* image_buffer,
                             float* out_color, int bounded, int debug, void* stream) {
  return forward_render(P, make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0),
                        render_out(nullptr, geom_buffer, num_rendered, binning_buffer, image_buffer, out_color),
                        bounded ? TAIL_BOUNDED : 0u, debug, (hipStream_t)stream);
}

int gs_forward_bounded(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                       const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, int prefiltered, int* radii_out, void* geom_buffer, long long capacity,
                       void* binning_buffer, void* image_buffer, float* out_color, int debug, void* stream) {
  return forward_view(
      make_scene(P, D, M, means3D, shs, shs_rest, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, prefiltered),
      FwdOut{radii_out, geom_buffer, capacity, binning_buffer, image_buffer, out_color}, Totals::Bounded, nullptr,
      debug, (hipStream_t)stream);
}

// The eager forward with its count read back at the end (gsrast.h): the ordering stores the totals
// into the readback slot and flags ERR_CAPACITY against `capacity`; the binning and the render are
// queued behind it on the stream at once, so the device never waits for the host's round trip.
int gs_forward_counted(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                       const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, int prefiltered, int* radii_out, void* geom_buffer, long long capacity,
                       void* binning_buffer, void* image_buffer, float* out_color, long long* num_rendered_host,
                       int debug, void* stream) {
  return forward_view(
      make_scene(P, D, M, means3D, shs, shs_rest, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, prefiltered),
      FwdOut{radii_out, geom_buffer, capacity, binning_buffer, image_buffer, out_color}, Totals::Counted,
      num_rendered_host, debug, (hipStream_t)stream);
}

// The K views' depth sorts as one set of launches (contiguous geometry buffers); GSRAST_BATCH_VIEWS=0
// in the environment runs them view by view on the views' streams (A/B runs; the Python layer then
// also bins the views one by one)
constexpr int GS_BATCH_ORDER_MAX = 2 << 20;      // Gaussians up to which the views' depth sorts batch
constexpr uint32_t GS_BATCH_BIN_MAX = 8u << 20;  // instances per view up to which gs_forward_bin_views batches
static bool batch_views() {
  static const bool on = [] {
    const char* e = getenv("GSRAST_BATCH_VIEWS");
    return !(e && e[0] == '0');
  }();
  return on;
}

// Fork events, one ring per thread and call site: a captured step may hold several forks
struct EventRing {
  hipEvent_t ev[4] = {};
  unsigned next = 0;
  hipEvent_t take() {  // the next slot's event (created on first use); null: error set
    hipEvent_t& e = ev[next++ & 3];
    if (!e && !check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate")) return nullptr;
    return e;
  }
};
static hipStream_t view_stream(void* const* vs, int v, hipStream_t st) { return vs && vs[v] ? (hipStream_t)vs[v] : st; }
// the views' later kernels run on their own streams, behind what `st` holds now
static void fork_to_view_streams(hipEvent_t fork, hipStream_t st, void* const* view_streams, int K) {
  check_hip(hipEventRecord(fork, st), "hipEventRecord");
  for (int v = 0; v < K; v++) {
    hipStream_t vs = view_stream(view_streams, v, st);
    if (vs != st) check_hip(hipStreamWaitEvent(vs, fork, 0), "hipStreamWaitEvent");
  }
}

// The per-view argument arrays of gs_forward_preprocess_views (K entries each)
struct ViewsIn {
  int K;
  const float* const* background;
  const int *image_width, *image_height;
  const float *const *viewmatrix, *const *projmatrix, *const *campos;
  const float *tan_fovx, *tan_fovy;
  int prefiltered;
  int* const* radii_out;
  void* const* geom_buffer;
  void* const* view_streams;
};

// capacity (bounded, gs_forward_preprocess_views_bounded): per-view binning capacities; the counts
// are not read back (num_rendered_host unused), a view over its capacity leaves the sticky flag
static int preprocess_views(const GaussianArgs& g, const ViewsIn& in, long long* num_rendered_host,
                            const long long* capacity, int debug, hipStream_t st) {
  const int K = in.K, P = g.P;
  clear_error(debug);
  if (K <= 0 || K > FUSED_MAX_VIEWS) return set_error("views: 1 to 8 per call"), 1;
  if (!in.background || !in.image_width || !in.image_height || !in.viewmatrix || !in.projmatrix || !in.campos ||
      !in.tan_fovx || !in.tan_fovy || !in.radii_out || !in.geom_buffer || (!num_rendered_host && !capacity))
    return set_error("missing per-view argument array"), 1;
  PreViews pv;
  pv.K = K;
  for (int v = 0; v < K; v++) {
    if (num_rendered_host) num_rendered_host[v] = 0;
    if (capacity && (capacity[v] < 0 || capacity[v] > GS_MAX_INSTANCES)) return set_error("capacity out of range"), 1;
    pv.c[v] = make_camera(in.background[v], in.image_width[v], in.image_height[v], in.viewmatrix[v], in.projmatrix[v],
                          in.campos[v], in.tan_fovx[v], in.tan_fovy[v], in.prefiltered);
    if (!validate(g, pv.c[v])) return 1;
    if (P > 0 && (!in.radii_out[v] || !in.geom_buffer[v])) return set_error("missing output pointer"), 1;
    pv.radii[v] = in.radii_out[v];
    geom_layout((size_t)P, &pv.geo[v], (char*)in.geom_buffer[v]);
  }
  if (P == 0) return 0;
  // (bounded: no readback slot, the views' flags go to the sticky words)
  ReadbackSlot* rb = capacity ? nullptr : readback_slot();
  BoundedStatus* bs = capacity ? bounded_status_checked() : nullptr;
  if (capacity ? !bs : !rb) return 1;
  static thread_local EventRing ring;
  hipEvent_t fork = ring.take();
  if (!fork) return 1;
  if (!capacity && check_order_flags(false)) return 1;  // earlier forwards' look-back waits (finished ones)
  uint32_t cap32[FUSED_MAX_VIEWS];
  for (int v = 0; v < K; v++) cap32[v] = capacity ? (uint32_t)capacity[v] : 0xFFFFFFFFu;
  // geometry buffers at one stride (slices of one allocation, as prepare_views makes them): the K
  // orderings run as one set of launches on `stream` (blockIdx.y = view), every view's totals
  // stored by the first histogram launch into readback words [8 v, 8 v + 4)
  void* const* gb = in.geom_buffer;
  const ptrdiff_t vstride = K > 1 ? (char*)gb[1] - (char*)gb[0] : 0;
  // (up to GS_BATCH_ORDER_MAX Gaussians: larger sorts fill the GPU on their own, and view by view
  // on the views' streams they overlap the other views' render kernels)
  bool batched = batch_views() && K > 1 && P <= GS_BATCH_ORDER_MAX && vstride >= (ptrdiff_t)gs_geom_buffer_bytes(P) &&
                 vstride % 256 == 0;
  for (int v = 2; v < K && batched; v++) batched = (char*)gb[v] == (char*)gb[0] + v * vstride;
  fwd_preprocess_views(g, pv, st);
  if (batched) {
    fwd_order(P, pv.geo[0], st, capacity ? nullptr : rb->dev, capacity ? nullptr : rb->ev[0], cap32,
              capacity ? bs->dev : nullptr, K, (uint64_t)vstride);
    // the views' later kernels run on their streams, after the orderings
    fork_to_view_streams(fork, st, in.view_streams, K);
  } else {
    // each view's ordering on its own stream (view_streams[v], or `stream`), after the preprocess
    fork_to_view_streams(fork, st, in.view_streams, K);
    for (int v = 0; v < K; v++) {
      hipStream_t vs = view_stream(in.view_streams, v, st);
      if (capacity)
        fwd_order(P, pv.geo[v], vs, nullptr, nullptr, &cap32[v], bs->dev);
      else
        fwd_order(P, pv.geo[v], vs, rb->dev + 8 * v, rb->ev[v]);
    }
  }
  if (capacity) return t_failed ? 1 : 0;
  for (int v = 0; v < (batched ? 1 : K); v++) check_hip(hipEventSynchronize(rb->ev[v]), "hipEventSynchronize");
  if (t_failed) return 1;
  if (check_order_flags()) return 1;  // the rest of the earlier forwards (behind their renders, as a rule)
  for (int v = 0; v < K; v++)
    if (!read_view_totals(rb->host + 8 * v, v, K, &num_rendered_host[v])) return 1;
  return 0;
}

int gs_forward_preprocess_views(int K, int P, int D, int M, const float* const* background, const int* image_width,
                                const int* image_height, const float* means3D, const float* shs,
                                const float* colors_precomp, const float* opacities, const float* scales,
                                float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                const float* const* viewmatrix, const float* const* projmatrix,
                                const float* const* campos, const float* tan_fovx, const float* tan_fovy,
                                int prefiltered, int* const* radii_out, void* const* geom_buffer,
                                long long* num_rendered_host, int debug, void* stream, void* const* view_streams) {
  if (!num_rendered_host) {
    clear_error(debug);
    return set_error("missing per-view argument array"), 1;
  }
  return preprocess_views(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      ViewsIn{K, background, image_width, image_height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
              prefiltered, radii_out, geom_buffer, view_streams},
      num_rendered_host, nullptr, debug, (hipStream_t)stream);
}

int gs_forward_preprocess_views_bounded(int K, int P, int D, int M, const float* const* background,
                                        const int* image_width, const int* image_height, const float* means3D,
                                        const float* shs, const float* colors_precomp, const float* opacities,
                                        const float* scales, float scale_modifier, const float* rotations,
                                        const float* cov3D_precomp, const float* const* viewmatrix,
                                        const float* const* projmatrix, const float* const* campos,
                                        const float* tan_fovx, const float* tan_fovy, int prefiltered,
                                        int* const* radii_out, void* const* geom_buffer, const long long* capacity,
                                        int debug, void* stream, void* const* view_streams) {
  if (!capacity) {
    clear_error(debug);
    return set_error("missing capacity array"), 1;
  }
  return preprocess_views(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      ViewsIn{K, background, image_width, image_height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
              prefiltered, radii_out, geom_buffer, view_streams},
      nullptr, capacity, debug, (hipStream_t)stream);
}

int gs_forward_bin_views(int K, int P, int W, int H, void* const* geom_buffer, const long long* num_rendered,
                         void* const* binning_buffer, void* const* image_buffer, int debug, void* stream,
                         void* const* view_streams) {
  clear_error(debug);
  if (K <= 0 || K > FUSED_MAX_VIEWS) return set_error("views: 1 to 8 per call"), 1;
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (W <= 0 || H <= 0) return set_error("image size must be positive"), 1;
  if (size_limit_error(W, H)) return 1;
  if (!geom_buffer || !num_rendered || !binning_buffer || !image_buffer) return set_error("missing per-view array"), 1;
  if (P == 0) return 0;
  long long I = 0;
  for (int v = 0; v < K; v++) {
    if (!geom_buffer[v] || !binning_buffer[v] || !image_buffer[v]) return set_error("view %d: missing buffer", v), 1;
    if (num_rendered[v] < 0 || num_rendered[v] > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
    I = num_rendered[v] > I ? num_rendered[v] : I;
  }
  hipStream_t st = (hipStream_t)stream;
  const CameraArgs c = size_camera(W, H);
  // every view's buffers at one stride per kind (slices of one allocation each)
  auto stride_of = [&](void* const* b, size_t min_bytes, uint64_t* out) {
    const ptrdiff_t d = K > 1 ? (char*)b[1] - (char*)b[0] : 0;
    if (K > 1 && (d < (ptrdiff_t)min_bytes || d % 256 != 0)) return false;
    for (int v = 2; v < K; v++)
      if ((char*)b[v] != (char*)b[0] + v * d) return false;
    *out = (uint64_t)d;
    return true;
  };
  uint64_t gs = 0, bs = 0, is = 0;
  if (!stride_of(geom_buffer, gs_geom_buffer_bytes(P), &gs) ||
      !stride_of(binning_buffer, gs_binning_buffer_bytes(I, W, H), &bs) ||
      !stride_of(image_buffer, gs_image_buffer_bytes(W, H), &is))
    return set_error("bin_views: each kind of buffer must be K slices of one allocation, one stride apart, each "
                     "sized for the largest num_rendered"), 1;
  if (!batch_views() || I > (long long)GS_BATCH_BIN_MAX) {
    // large views: each view's binning on its own stream, where it overlaps the other views'
    // render kernels (a batched sort of K large views would serialise in front of them)
    for (int v = 0; v < K; v++) {
      const Layouts L(P, I, c, geom_buffer[v], binning_buffer[v], image_buffer[v]);
      fwd_bin_views(1, P, (uint32_t)I, c, L.geo, L.bin, L.img, 0, 0, 0, view_stream(view_streams, v, st));
    }
    return t_failed ? 1 : 0;
  }
  const Layouts L(P, I, c, geom_buffer[0], binning_buffer[0], image_buffer[0]);
  fwd_bin_views(K, P, (uint32_t)I, c, L.geo, L.bin, L.img, gs, bs, is, st);
  // the views' renders run on their streams, after the binning
  static thread_local EventRing ring;
  hipEvent_t done = ring.take();
  if (!done) return 1;
  fork_to_view_streams(done, st, view_streams, K);
  return t_failed ? 1 : 0;
}

int gs_bounded_status(unsigned* flags, long long* instances) {
  clear_error(0);
  BoundedStatus* bs = bounded_status();
  if (!bs) return 1;
  long long inst = 0;
  const uint32_t f = take_bounded_status(bs, &inst);
  if (flags) *flags = f;
  if (instances) *instances = inst;
  return bounded_status_error(f, inst) ? 1 : 0;
}

size_t gs_geom_flags_offset(int P) {
  // the layout's offsets from a dummy base address (nothing is dereferenced)
  alignas(256) static char base[256];
  GeomPtrs geo;
  geom_layout((size_t)(P > 0 ? P : 1), &geo, base);
  return (size_t)((uintptr_t)geo.counters - (uintptr_t)base) + CNT_ERR * sizeof(uint32_t);
}

int gs_forward_order_status(void) {
  clear_error(0);
  return check_order_flags(true) ? 1 : 0;
}

int gs_set_row_waits(int n, const int* bounds, void* const* events) {
  clear_error(0);
  t_row_wait_count = 0;
  if (n == 0) return 0;
  if (n < 0 || n > GS_MAX_ROW_WAITS) return set_error("row waits: 0..%d chunks (got %d)", GS_MAX_ROW_WAITS, n), 1;
  if (!bounds || !events) return set_error("row waits: missing bounds / events"), 1;
  if (bounds[0] != 0) return set_error("row waits: the first chunk must start at row 0"), 1;
  for (int k = 0; k < n; k++)
    if (bounds[k + 1] <= bounds[k]) return set_error("row waits: chunk bounds must increase"), 1;
  for (int k = 0; k < n; k++) t_row_waits[k] = RowWait{bounds[k + 1], (hipEvent_t)events[k]};
  t_row_wait_count = n;
  return 0;
}

long long gs_rasterize_forward(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                               const float* shs, const float* colors_precomp, const float* opacities,
                               const float* scales, float scale_modifier, const float* rotations,
                               const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                               const float* campos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                               int* radii_out, gs_alloc_fn alloc, void* alloc_ctx, void** geom_out,
                               void** binning_out, void** image_out, int debug, void* stream) {
  if (!alloc) {
    clear_error(debug);
    set_error("alloc callback is NULL");
    return -1;
  }
  void* geom = alloc(alloc_ctx, 0, gs_geom_buffer_bytes(P));
  long long I = 0;
  if (gs_forward_preprocess(P, D, M, background, W, H, means3D, shs, colors_precomp, opacities, scales,
                            scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                            tan_fovy, prefiltered, radii_out, geom, &I, debug, stream))
    return -1;
  void* bin = alloc(alloc_ctx, 1, gs_binning_buffer_bytes(I, W, H));
  void* img = alloc(alloc_ctx, 2, gs_image_buffer_bytes(W, H));
  if (geom_out) *geom_out = geom;
  if (binning_out) *binning_out = bin;
  if (image_out) *image_out = img;
  if (gs_forward_render(P, background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii_out, geom, I,
                        bin, img, out_color, debug, stream))
    return -1;
  return I;
}

// ---- backward: the same packing (make_scene, make_camera, BwdIn, GradOut) ----
// What a view's backward reads besides the scene, and its scratch
struct BwdIn {
  const void* geom;
  long long num_rendered;
  const void* binning;
  const void* image;
  const float* dL_dout_color;
  void* grad_buffer;
  const float* dL_dout_invdepth = nullptr;  // gs_backward_accumulate_aux (either may be null)
  const float* dL_dout_alpha = nullptr;
  bool antialiasing = false;  // gs_backward_accumulate_aa: the forward scaled the opacities (needs g.opacities)
  float* dL_dmeans2D_abs = nullptr;  // gs_backward_accumulate_absgrad: [P, 3], or null (the call without it)
};

// out: the caller's gradient pointers as passed; the ones the scene's inputs cannot receive are dropped here
static int backward_impl(const GaussianArgs& g, const CameraArgs& c, const BwdIn& in, GradOut out, void* wait_event,
                         int debug, hipStream_t st) {
  const int P = g.P;
  const long long num_rendered = in.num_rendered;
  clear_error(debug);
  // (the opacity is carried by the forward's splat records: not required here; an antialiased
  // backward chains through the scale and reads it)
  if (!validate(g, c, in.antialiasing)) return 1;
  if (P == 0) return 0;
  if (!in.geom || !in.binning || !in.image || !in.dL_dout_color || !in.grad_buffer)
    return set_error("missing buffer pointer"), 1;
  if (!out.dmean2D || !out.dopacity || !out.dmean3D) return set_error("missing gradient output pointer"), 1;
  // SH colours chain into dL/dmeans3D through the view direction inside the kernels that form dL/dsh:
  // without that output the colours kernel would run and leave the term out
  if (g.shs && !out.dsh) return set_error("dL_dsh is required with SHs"), 1;
  if (num_rendered < 0 || num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
  if (out.acc & ~0xFFu) return set_error("accumulate: unknown GS_ACC bits 0x%x", out.acc), 1;
  const Layouts L(P, num_rendered, c, in.geom, in.binning, in.image);
  float* gradrec = (float*)in.grad_buffer;
  // an aux gradient (gs_backward_accumulate_aux): the side arrays behind the records; none: the plain path
  BwdAux aux;
  if (in.dL_dout_invdepth || in.dL_dout_alpha) {
    size_t o_rec = 0, o_sum = 0;
    grad_layout_aux((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)P, &o_rec, &o_sum);
    aux.d_invdepth = in.dL_dout_invdepth;
    aux.d_alpha = in.dL_dout_alpha;
    aux.gradrec_aux = (float*)((char*)in.grad_buffer + o_rec);
    aux.gsum_aux = (float*)((char*)in.grad_buffer + o_sum);
  }
  // the absolute screen-space sums (gs_backward_accumulate_absgrad): their side arrays behind the aux layout
  BwdAbs ab;
  if (in.dL_dmeans2D_abs) {
    size_t o_rec = 0, o_sum = 0;
    grad_layout_abs((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)P, &o_rec, &o_sum);
    ab.gradrec_abs = (float*)((char*)in.grad_buffer + o_rec);
    ab.gsum_abs = (float*)((char*)in.grad_buffer + o_sum);
  }
  if (num_rendered > 0) bwd_render(P, c, L.geo, L.bin, L.img, in.dL_dout_color, gradrec, st, aux, ab);
  // dL_dcov3D is filled whenever the caller passes it: upstream writes it for scale/rotation
  // inputs too (the covariance gradient the scale / rotation chain starts from)
  if (!g.shs) out.dsh = nullptr;
  if (g.cov3D) out.dscale = out.drot = nullptr;
  // the gradient outputs may be shared with views on other streams: order only this last kernel
  if (wait_event && !check_hip(hipStreamWaitEvent(st, (hipEvent_t)wait_event, 0), "hipStreamWaitEvent")) return 1;
  bwd_preprocess(g, c, L.geo, L.bin, L.img, gradrec, (uint32_t)num_rendered, num_rendered > 0, out, st, aux,
                 in.antialiasing, ab);
  // (without instances no Gaussian has a tile: zero rows, the sums are not read)
  if (ab.on()) bwd_absgrad(P, c, L.geo, ab, in.dL_dmeans2D_abs, st);
  if (aux.on() && num_rendered > 0) {
    // the depth chain's term, added after the kernel that wrote dL_dmeans3D (same stream, behind the wait)
    bwd_depth_chain(g, c, L.geo, aux, out.dmean3D, st);
  }
  // the ordering flags of the forwards that have finished, now that this backward's kernels are queued
  if (!t_failed && check_order_flags(false)) return 1;
  return t_failed ? 1 : 0;
}

int gs_backward(int P, int D, int M, const float* background, int W, int H, const float* means3D, const float* shs,
                const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                long long num_rendered, const void* binning_buffer, const void* image_buffer,
                const float* dL_dout_color, void* grad_buffer, float* dL_dmeans2D, float* dL_dcolors,
                float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                float* dL_drotations, int debug, void* stream) {
  return gs_backward_accumulate(P, D, M, background, W, H, means3D, shs, colors_precomp, opacities, scales,
                                scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                                tan_fovy, radii, geom_buffer, num_rendered, binning_buffer, image_buffer,
                                dL_dout_color, grad_buffer, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D,
                                dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, 0u, nullptr, debug, stream);
}

int gs_backward_accumulate(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                           const float* shs, const float* colors_precomp, const float* opacities,
                           const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                           const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                           const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                           const void* image_buffer, const float* dL_dout_color, void* grad_buffer,
                           float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                           float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                           unsigned accumulate, void* wait_event, int debug, void* stream) {
  return gs_backward_accumulate_absgrad(P, D, M, background, W, H, means3D, shs, nullptr, colors_precomp, opacities,
                                        scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                        campos, tan_fovx, tan_fovy, radii, geom_buffer, num_rendered, binning_buffer,
                                        image_buffer, dL_dout_color, nullptr, nullptr, grad_buffer, dL_dmeans2D,
                                        dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
                                        dL_drotations, accumulate, wait_event, debug, stream, 0, nullptr);
}

int gs_backward_accumulate_aux(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                               const float* shs, const float* shs_rest, const float* colors_precomp,
                               const float* opacities, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                               const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                               const int* radii, const void* geom_buffer, long long num_rendered,
                               const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                               const float* dL_dout_invdepth, const float* dL_dout_alpha, void* grad_buffer,
                               float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                               float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                               unsigned accumulate, void* wait_event, int debug, void* stream) {
  return gs_backward_accumulate_absgrad(P, D, M, background, W, H, means3D, shs, shs_rest, colors_precomp, opacities,
                                        scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                        campos, tan_fovx, tan_fovy, radii, geom_buffer, num_rendered, binning_buffer,
                                        image_buffer, dL_dout_color, dL_dout_invdepth, dL_dout_alpha, grad_buffer,
                                        dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                                        dL_dscales, dL_drotations, accumulate, wait_event, debug, stream, 0, nullptr);
}

int gs_backward_accumulate_aa(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                              const float* shs, const float* shs_rest, const float* colors_precomp,
                              const float* opacities, const float* scales, float scale_modifier,
                              const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                              const int* radii, const void* geom_buffer, long long num_rendered,
                              const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                              const float* dL_dout_invdepth, const float* dL_dout_alpha, void* grad_buffer,
                              float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                              float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                              unsigned accumulate, void* wait_event, int debug, void* stream, int antialiasing) {
  return gs_backward_accumulate_absgrad(P, D, M, background, W, H, means3D, shs, shs_rest, colors_precomp, opacities,
                                        scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                        campos, tan_fovx, tan_fovy, radii, geom_buffer, num_rendered, binning_buffer,
                                        image_buffer, dL_dout_color, dL_dout_invdepth, dL_dout_alpha, grad_buffer,
                                        dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                                        dL_dscales, dL_drotations, accumulate, wait_event, debug, stream, antialiasing,
                                        nullptr);
}

int gs_backward_accumulate_absgrad(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                                   const float* shs, const float* shs_rest, const float* colors_precomp,
                                   const float* opacities, const float* scales, float scale_modifier,
                                   const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                   const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                                   const int* radii, const void* geom_buffer, long long num_rendered,
                                   const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                                   const float* dL_dout_invdepth, const float* dL_dout_alpha, void* grad_buffer,
                                   float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                                   float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                   unsigned accumulate, void* wait_event, int debug, void* stream, int antialiasing,
                                   float* dL_dmeans2D_abs) {
  (void)radii;
  if (antialiasing && shs_rest) {
    clear_error(debug);
    return set_error("antialiasing: not supported with split SH rows (shs_rest)"), 1;
  }
  BwdIn in{geom_buffer, num_rendered, binning_buffer, image_buffer, dL_dout_color, grad_buffer, dL_dout_invdepth,
           dL_dout_alpha};
  in.antialiasing = antialiasing != 0;
  in.dL_dmeans2D_abs = dL_dmeans2D_abs;
  return backward_impl(
      make_scene(P, D, M, means3D, shs, shs_rest, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0), in,
      GradOut{dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
              accumulate},
      wait_event, debug, (hipStream_t)stream);
}

int gs_backward_accumulate_split(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                                 const float* shs_dc, const float* shs_rest, const float* opacities,
                                 const float* scales, float scale_modifier, const float* rotations,
                                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                 const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                                 const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                                 const void* image_buffer, const float* dL_dout_color, void* grad_buffer,
                                 float* dL_dmeans2D, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                                 float* dL_dsh, float* dL_dscales, float* dL_drotations, unsigned accumulate,
                                 void* wait_event, int debug, void* stream) {
  if (!shs_rest) {
    clear_error(debug);
    return set_error("split SH: features_rest is NULL"), 1;
  }
  return gs_backward_accumulate_absgrad(P, D, M, background, W, H, means3D, shs_dc, shs_rest, nullptr, opacities,
                                        scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                        campos, tan_fovx, tan_fovy, radii, geom_buffer, num_rendered, binning_buffer,
                                        image_buffer, dL_dout_color, nullptr, nullptr, grad_buffer, dL_dmeans2D,
                                        nullptr, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
                                        dL_drotations, accumulate, wait_event, debug, stream, 0, nullptr);
}

size_t gs_camera_grad_scratch_bytes(int P) { return camera_grad_scratch_bytes((size_t)(P > 0 ? P : 0)); }

// The camera gradient of one view behind its backward (gs_backward_camera; aa: gs_backward_camera_aa,
// whose kernels read the opacities)
static int backward_camera_impl(const GaussianArgs& g, const CameraArgs& c, const void* geom_buffer,
                                long long num_rendered, const void* aux_grad_buffer, int aux_valid, void* scratch,
                                float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, int debug,
                                hipStream_t st, bool aa) {
  const int P = g.P;
  clear_error(debug);
  if (!validate(g, c, aa)) return 1;
  if (!dL_dviewmatrix || !dL_dprojmatrix) return set_error("missing gradient output pointer"), 1;
  if (P == 0) {  // no Gaussians: zero gradients
    if (!check_hip(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), st), "hipMemsetAsync") ||
        !check_hip(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), st), "hipMemsetAsync") ||
        (dL_dcampos && !check_hip(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), st), "hipMemsetAsync")))
      return 1;
    return 0;
  }
  if (!geom_buffer || !scratch || (aux_valid && !aux_grad_buffer)) return set_error("missing buffer pointer"), 1;
  if (((uintptr_t)scratch) & 15) return set_error("camera grad: scratch must be 16-byte aligned"), 1;
  if (num_rendered < 0 || num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
  GeomPtrs geo;
  geom_layout((size_t)P, &geo, (char*)geom_buffer);
  const float* gsum_aux = nullptr;
  if (aux_valid) {
    size_t o_sum = 0;
    grad_layout_aux((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)P, nullptr, &o_sum);
    gsum_aux = (const float*)((const char*)aux_grad_buffer + o_sum);
  }
  // (without instances the aux backward sums nothing: no depth term, as in backward_impl)
  bwd_camera(g, c, geo, num_rendered > 0 ? gsum_aux : nullptr, (double*)scratch, dL_dviewmatrix, dL_dprojmatrix,
             dL_dcampos, st, aa);
  return t_failed ? 1 : 0;
}

int gs_backward_camera(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                       const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, const void* geom_buffer, long long num_rendered, const void* aux_grad_buffer,
                       int aux_valid, void* scratch, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                       int debug, void* stream) {
  return gs_backward_camera_aa(P, D, M, background, W, H, means3D, shs, colors_precomp, opacities, scales,
                               scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                               tan_fovy, geom_buffer, num_rendered, aux_grad_buffer, aux_valid, scratch,
                               dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, debug, stream, 0);
}

int gs_backward_camera_aa(int P, int D, int M, const float* background, int W, int H, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* opacities,
                          const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* campos, float tan_fovx, float tan_fovy, const void* geom_buffer,
                          long long num_rendered, const void* aux_grad_buffer, int aux_valid, void* scratch,
                          float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, int debug, void* stream,
                          int antialiasing) {
  return backward_camera_impl(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, opacities, scales, scale_modifier, rotations,
                 cov3D_precomp),
      make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0), geom_buffer,
      num_rendered, aux_grad_buffer, aux_valid, scratch, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, debug,
      (hipStream_t)stream, antialiasing != 0);
}

int gs_backward_render(int P, int D, int M, const float* background, int W, int H, const float* viewmatrix,
                       const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                       const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                       const void* image_buffer, const float* dL_dout_color, void* grad_buffer, float* dL_dmeans2D,
                       unsigned accumulate, int debug, void* stream) {
  return gs_backward_render_aux(P, D, M, background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                                geom_buffer, num_rendered, binning_buffer, image_buffer, dL_dout_color, nullptr,
                                nullptr, grad_buffer, dL_dmeans2D, nullptr, accumulate, debug, stream);
}

int gs_backward_render_aux(int P, int D, int M, const float* background, int W, int H, const float* viewmatrix,
                           const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                           const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                           const void* image_buffer, const float* dL_dout_color, const float* dL_dout_invdepth,
                           const float* dL_dout_alpha, void* grad_buffer, float* dL_dmeans2D, float* invdepth_sums,
                           unsigned accumulate, int debug, void* stream) {
  const CameraArgs c = make_camera(background, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0);
  clear_error(debug);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (W <= 0 || H <= 0) return set_error("image size must be positive (got %d x %d)", W, H), 1;
  if (size_limit_error(W, H)) return 1;
  if (P == 0) return 0;
  if (!viewmatrix || !projmatrix || !background) return set_error("missing required input pointer"), 1;
  const bool with_aux = dL_dout_invdepth || dL_dout_alpha;
  if (!geom_buffer || !binning_buffer || !image_buffer || !dL_dout_color || !grad_buffer ||
      (with_aux && !invdepth_sums))
    return set_error("missing buffer pointer"), 1;
  if (num_rendered < 0 || num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
  if (accumulate & ~GS_ACC_MEANS2D) return set_error("accumulate: only GS_ACC_MEANS2D applies here"), 1;
  hipStream_t st = (hipStream_t)stream;
  const Layouts L(P, num_rendered, c, geom_buffer, binning_buffer, image_buffer);
  // (the record sums read the scene's sizes only)
  const GaussianArgs g = make_scene(P, D, M, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0f, nullptr,
                                    nullptr);
  float* gradrec = (float*)grad_buffer;
  // an aux gradient: the instances' side array behind the records (gs_grad_buffer_bytes_aux; its
  // per-Gaussian tail is unused), the per-Gaussian sums in the caller's array; none: the plain path
  BwdAux aux;
  if (with_aux) {
    size_t o_rec = 0;
    grad_layout_aux((size_t)(num_rendered > 0 ? num_rendered : 1), (size_t)P, &o_rec, nullptr);
    aux.d_invdepth = dL_dout_invdepth;
    aux.d_alpha = dL_dout_alpha;
    aux.gradrec_aux = (float*)((char*)grad_buffer + o_rec);
    aux.gsum_aux = invdepth_sums;
  }
  if (num_rendered > 0) bwd_render(P, c, L.geo, L.bin, L.img, dL_dout_color, gradrec, st, aux);
  bwd_records(g, L.geo, L.bin, L.img, gradrec, (uint32_t)num_rendered, num_rendered > 0, dL_dmeans2D, accumulate, st,
              aux);
  if (!t_failed && check_order_flags(false)) return 1;
  return t_failed ? 1 : 0;
}

size_t gs_contrib_scratch_bytes(long long num_rendered) {
  return contrib_scratch_bytes((size_t)(num_rendered > 0 ? num_rendered : 0));
}

int gs_contrib_stats(int P, int W, int H, const float* viewmatrix, const float* projmatrix, const float* campos,
                     float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                     long long num_rendered, const void* binning_buffer, void* image_buffer,
                     const float* pixel_weights, void* scratch, float* wsum, float* wmax, int* count,
                     int accumulate, int debug, void* stream) {
  (void)radii;
  clear_error(debug);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (W <= 0 || H <= 0) return set_error("image size must be positive (got %d x %d)", W, H), 1;
  if (size_limit_error(W, H)) return 1;
  if (!wsum && !wmax && !count) return set_error("missing output pointer"), 1;
  if (num_rendered < 0 || num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), 1;
  if (P == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (num_rendered == 0) {  // no instance: zero statistics (nothing to add when accumulating)
    if (accumulate) return 0;
    const size_t bytes = sizeof(float) * (size_t)P;
    if ((wsum && !check_hip(hipMemsetAsync(wsum, 0, bytes, st), "hipMemsetAsync")) ||
        (wmax && !check_hip(hipMemsetAsync(wmax, 0, bytes, st), "hipMemsetAsync")) ||
        (count && !check_hip(hipMemsetAsync(count, 0, bytes, st), "hipMemsetAsync")))
      return 1;
    return 0;
  }
  if (!geom_buffer || !binning_buffer || !image_buffer || !scratch) return set_error("missing buffer pointer"), 1;
  const CameraArgs c = make_camera(nullptr, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0);
  const Layouts L(P, num_rendered, c, geom_buffer, binning_buffer, image_buffer);
  contrib_stats(P, c, L.geo, L.bin, L.img, pixel_weights, scratch, wsum, wmax, count, accumulate != 0, st);
  if (!t_failed && check_order_flags(false)) return 1;
  return t_failed ? 1 : 0;
}

int gs_feature_group_channels(void) { return GS_FEATURE_GROUP; }

size_t gs_feature_scratch_bytes(long long num_rendered) {
  return feature_scratch_bytes((size_t)(num_rendered > 0 ? num_rendered : 0));
}

// the checks the two feature entries share, in the header's order (before any device work)
static bool feature_args_error(int P, int C, int W, int H, long long num_rendered) {
  if (P < 0) return set_error("P must be >= 0"), true;
  if (C < 1 || C > GS_MAX_FEATURE_CHANNELS)
    return set_error("feature channels must lie in [1, %d] (got %d)", GS_MAX_FEATURE_CHANNELS, C), true;
  if (W <= 0 || H <= 0) return set_error("image size must be positive (got %d x %d)", W, H), true;
  if (size_limit_error(W, H)) return true;
  if (num_rendered < 0 || num_rendered > GS_MAX_INSTANCES) return set_error("num_rendered out of range"), true;
  return false;
}

int gs_feature_forward(int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                       const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                       const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                       void* image_buffer, const float* features, float* out, int debug, void* stream) {
  (void)radii;
  clear_error(debug);
  if (feature_args_error(P, C, W, H, num_rendered)) return 1;
  if (!out) return set_error("missing output pointer"), 1;
  hipStream_t st = (hipStream_t)stream;
  if (P == 0 || num_rendered == 0)  // no instance: a zero image
    return check_hip(hipMemsetAsync(out, 0, sizeof(float) * (size_t)C * (size_t)W * (size_t)H, st), "hipMemsetAsync")
               ? 0
               : 1;
  if (!geom_buffer || !binning_buffer || !image_buffer || !features) return set_error("missing buffer pointer"), 1;
  const CameraArgs c = make_camera(nullptr, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0);
  const Layouts L(P, num_rendered, c, geom_buffer, binning_buffer, image_buffer);
  feature_forward(P, C, c, L.geo, L.bin, L.img, features, out, st);
  if (!t_failed && check_order_flags(false)) return 1;
  return t_failed ? 1 : 0;
}

int gs_feature_backward(int P, int C, int W, int H, const float* viewmatrix, const float* projmatrix,
                        const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                        const void* geom_buffer, long long num_rendered, const void* binning_buffer,
                        void* image_buffer, const float* dL_dout, void* scratch, float* dL_dfeatures,
                        int accumulate, int debug, void* stream) {
  (void)radii;
  clear_error(debug);
  if (feature_args_error(P, C, W, H, num_rendered)) return 1;
  if (P == 0) return 0;
  if (!dL_dfeatures) return set_error("missing output pointer"), 1;
  hipStream_t st = (hipStream_t)stream;
  if (num_rendered == 0) {  // no instance: zero gradients (nothing to add when accumulating)
    if (accumulate) return 0;
    return check_hip(hipMemsetAsync(dL_dfeatures, 0, sizeof(float) * (size_t)P * (size_t)C, st), "hipMemsetAsync")
               ? 0
               : 1;
  }
  if (!geom_buffer || !binning_buffer || !image_buffer || !dL_dout || !scratch)
    return set_error("missing buffer pointer"), 1;
  if ((uintptr_t)scratch & 15u) return set_error("scratch must be 16-byte aligned"), 1;
  const CameraArgs c = make_camera(nullptr, W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, 0);
  const Layouts L(P, num_rendered, c, geom_buffer, binning_buffer, image_buffer);
  feature_backward(P, C, c, L.geo, L.bin, L.img, dL_dout, scratch, dL_dfeatures, accumulate != 0, st);
  if (!t_failed && check_order_flags(false)) return 1;
  return t_failed ? 1 : 0;
}

// scene, grads: the whole scene and the caller's gradient pointers (P rows), of which [first, first + count) run
static int backward_gaussians_impl(const GaussianArgs& scene, int first, int count, int num_views,
                                   const gs_view_grad* views, const GradOut& grads, void* wait_event, int debug,
                                   hipStream_t st) {
  const int P = scene.P;
  clear_error(debug);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (first < 0 || count < 0 || (long long)first + count > P) return set_error("Gaussian range out of bounds"), 1;
  if (num_views < 0 || (num_views > 0 && !views)) return set_error("bad view list"), 1;
  if (P == 0 || count == 0 || num_views == 0) return 0;
  if (!scene.means3D) return set_error("missing required input pointer"), 1;
  if ((scene.shs == nullptr) == (scene.colors == nullptr))
    return set_error("Please provide excatly one of either SHs or precomputed colors!"), 1;
  if (((scene.scales == nullptr || scene.rotations == nullptr) && scene.cov3D == nullptr) ||
      ((scene.scales || scene.rotations) && scene.cov3D))
    return set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"), 1;
  if (scene.shs && (scene.D < 0 || scene.D > 3 || scene.M < (scene.D + 1) * (scene.D + 1)))
    return set_error("bad SH degree / coefficient count"), 1;
  if (!grads.dopacity || !grads.dmean3D) return set_error("missing gradient output pointer"), 1;
  if (scene.shs && !grads.dsh) return set_error("dL_dsh is required with SHs"), 1;  // (as backward_impl)
  if (grads.acc & ~0xFFu) return set_error("accumulate: unknown GS_ACC bits 0x%x", grads.acc), 1;
  for (int v = 0; v < num_views; v++) {
    const gs_view_grad& w = views[v];
    if (!w.viewmatrix || !w.projmatrix || !w.geom_buffer || (scene.shs && !w.campos))
      return set_error("view %d: missing pointer", v), 1;
    if (w.image_width <= 0 || w.image_height <= 0) return set_error("view %d: bad image size", v), 1;
    char pre[32];
    snprintf(pre, sizeof(pre), "view %d: ", v);
    if (size_limit_error(w.image_width, w.image_height, pre)) return 1;
  }
  if (wait_event && !check_hip(hipStreamWaitEvent(st, (hipEvent_t)wait_event, 0), "hipStreamWaitEvent")) return 1;
  // the range [first, first + count) as a P = count problem: every per-Gaussian array is row-indexed,
  // so the rows' pointers are offset by `first` (the geom buffers keep their P-row layout)
  const size_t f = (size_t)first, M = (size_t)scene.M;
  auto off = [f](const float* p, size_t w) { return p ? p + f * w : nullptr; };
  auto offw = [f](float* p, size_t w) { return p ? p + f * w : nullptr; };
  const GaussianArgs g = make_scene(count, scene.D, scene.M, off(scene.means3D, 3), off(scene.shs, 3 * M), nullptr,
                                    off(scene.colors, 3), nullptr, off(scene.scales, 3), scene.scale_modifier,
                                    off(scene.rotations, 4), off(scene.cov3D, 6));
  // passes of up to FUSED_MAX_VIEWS views; the later passes add to what the earlier wrote
  for (int v0 = 0; v0 < num_views; v0 += FUSED_MAX_VIEWS) {
    FusedViews fv;
    fv.K = num_views - v0 < FUSED_MAX_VIEWS ? num_views - v0 : FUSED_MAX_VIEWS;
    for (int k = 0; k < fv.K; k++) {
      const gs_view_grad& w = views[v0 + k];
      GeomPtrs geo;
      geom_layout((size_t)P, &geo, (char*)w.geom_buffer);
      fv.v[k].c = make_camera(nullptr, w.image_width, w.image_height, w.viewmatrix, w.projmatrix, w.campos,
                              w.tan_fovx, w.tan_fovy, 0);
      fv.v[k].tiles = geo.tiles + f;
      fv.v[k].clamped = geo.clamped + f;
      fv.v[k].gsum = geo.gsum + f * GRAD_REC;
    }
    const GradOut out{nullptr, offw(grads.dcolor, 3), offw(grads.dopacity, 1), offw(grads.dmean3D, 3),
                      offw(grads.dcov3D, 6), scene.shs ? offw(grads.dsh, 3 * M) : nullptr,
                      scene.cov3D ? nullptr : offw(grads.dscale, 3), scene.cov3D ? nullptr : offw(grads.drot, 4),
                      v0 == 0 ? grads.acc : 0xFFu};
    bwd_gaussians(g, fv, out, st);
  }
  return t_failed ? 1 : 0;
}

int gs_backward_gaussians(int P, int D, int M, const float* means3D, const float* shs, const float* colors_precomp,
                          const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, int num_views, const gs_view_grad* views, float* dL_dcolors,
                          float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                          float* dL_dscales, float* dL_drotations, unsigned accumulate, void* wait_event, int debug,
                          void* stream) {
  return gs_backward_gaussians_range(P, 0, P, D, M, means3D, shs, colors_precomp, scales, scale_modifier, rotations,
                                     cov3D_precomp, num_views, views, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D,
                                     dL_dsh, dL_dscales, dL_drotations, accumulate, wait_event, debug, stream);
}

int gs_backward_gaussians_range(int P, int first, int count, int D, int M, const float* means3D, const float* shs,
                                const float* colors_precomp, const float* scales, float scale_modifier,
                                const float* rotations, const float* cov3D_precomp, int num_views,
                                const gs_view_grad* views, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                                float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                                unsigned accumulate, void* wait_event, int debug, void* stream) {
  return backward_gaussians_impl(
      make_scene(P, D, M, means3D, shs, nullptr, colors_precomp, nullptr, scales, scale_modifier, rotations,
                 cov3D_precomp),
      first, count, num_views, views,
      GradOut{nullptr, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, accumulate},
      wait_event, debug, (hipStream_t)stream);
}

int gs_backward_gaussians_adam(int P, int D, int M, const float* means3D, const float* shs_dc, const float* shs_rest,
                               const float* scales, float scale_modifier, const float* rotations,
                               const gs_view_grad* view, float* const* params_host, float* const* exp_avg_host,
                               float* const* exp_avg_sq_host, const double* lr_host, const long long* step_host,
                               const double* weight_decay_host, double beta1, double beta2, double eps, int maximize,
                               int debug, void* stream) {
  return gs_backward_gaussians_adam_stats(P, D, M, means3D, shs_dc, shs_rest, scales, scale_modifier, rotations, view,
                                          params_host, exp_avg_host, exp_avg_sq_host, lr_host, step_host,
                                          weight_decay_host, beta1, beta2, eps, maximize, nullptr, nullptr, 0, nullptr,
                                          nullptr, nullptr, debug, stream);
}

int gs_backward_gaussians_adam_stats(int P, int D, int M, const float* means3D, const float* shs_dc,
                                     const float* shs_rest, const float* scales, float scale_modifier,
                                     const float* rotations, const gs_view_grad* view, float* const* params_host,
                                     float* const* exp_avg_host, float* const* exp_avg_sq_host, const double* lr_host,
                                     const long long* step_host, const double* weight_decay_host, double beta1,
                                     double beta2, double eps, int maximize, const int* radii, const float* grad2d,
                                     int grad_stride, float* max_radii2D, float* grad_accum, float* denom, int debug,
                                     void* stream) {
  return gs_backward_gaussians_adam_stats_aux(P, D, M, means3D, shs_dc, shs_rest, scales, scale_modifier, rotations,
                                              view, params_host, exp_avg_host, exp_avg_sq_host, lr_host, step_host,
                                              weight_decay_host, beta1, beta2, eps, maximize, radii, grad2d,
                                              grad_stride, max_radii2D, grad_accum, denom, nullptr, debug, stream);
}

int gs_backward_gaussians_adam_stats_aux(int P, int D, int M, const float* means3D, const float* shs_dc,
                                         const float* shs_rest, const float* scales, float scale_modifier,
                                         const float* rotations, const gs_view_grad* view,
                                         float* const* params_host, float* const* exp_avg_host,
                                         float* const* exp_avg_sq_host, const double* lr_host,
                                         const long long* step_host, const double* weight_decay_host, double beta1,
                                         double beta2, double eps, int maximize, const int* radii,
                                         const float* grad2d, int grad_stride, float* max_radii2D, float* grad_accum,
                                         float* denom, const float* invdepth_sums, int debug, void* stream) {
  clear_error(debug);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (P == 0) return 0;
  if (D < 0 || D > 3 || M != 16) return set_error("fused Adam backward: 16 SH coefficients, degree 0..3 only"), 1;
  if (!means3D || !shs_dc || !shs_rest || !scales || !rotations || !view || !params_host || !exp_avg_host ||
      !exp_avg_sq_host || !lr_host || !step_host)
    return set_error("missing required input pointer"), 1;
  if (!view->viewmatrix || !view->projmatrix || !view->campos || !view->geom_buffer)
    return set_error("view: missing pointer"), 1;
  if (view->image_width <= 0 || view->image_height <= 0) return set_error("view: bad image size"), 1;
  if (size_limit_error(view->image_width, view->image_height, "view: ")) return 1;
  for (int k = 0; k < 6; k++) {
    if (!params_host[k] || !exp_avg_host[k] || !exp_avg_sq_host[k]) return set_error("missing tensor pointer"), 1;
    if (step_host[k] < 1) return set_error("adam: step must be >= 1"), 1;
  }
  if (means3D != params_host[DT_XYZ]) return set_error("means3D must be the xyz parameter (params_host[0])"), 1;
  if (((uintptr_t)params_host[DT_ROT]) & 15) return set_error("rotation parameter must be 16-byte aligned"), 1;
  if ((((uintptr_t)shs_dc) | ((uintptr_t)shs_rest)) & 15) return set_error("split SH rows must be 16-byte aligned"), 1;
  // the kernel's 16-B accesses (adam_sh_block, the rotation rows): the parameter and both moments of these groups
  static const struct { int k; const char* name; } vec_groups[] = {
      {DT_FDC, "features_dc"}, {DT_FREST, "features_rest"}, {DT_ROT, "rotation"}};
  for (const auto& vg : vec_groups)
    if ((((uintptr_t)params_host[vg.k]) | ((uintptr_t)exp_avg_host[vg.k]) | ((uintptr_t)exp_avg_sq_host[vg.k])) & 15)
      return set_error("fused Adam backward: %s parameter, exp_avg and exp_avg_sq must be 16-byte aligned", vg.name), 1;
  const GaussianArgs g = make_scene(P, D, M, means3D, shs_dc, shs_rest, nullptr, nullptr, scales, scale_modifier,
                                    rotations, nullptr);
  FusedAdamArgs a{};
  for (int k = 0; k < 6; k++) {
    a.p[k] = params_host[k];
    a.m[k] = exp_avg_host[k];
    a.v[k] = exp_avg_sq_host[k];
    adam_scalars(lr_host[k], step_host[k], beta1, beta2, &a.nss[k], &a.bc2s[k]);
    a.wd[k] = weight_decay_host ? (float)weight_decay_host[k] : 0.0f;
  }
  a.k = adam_consts(beta1, beta2, eps, maximize != 0);
  const bool any_stat = radii || grad2d || max_radii2D || grad_accum || denom;
  if (any_stat) {
    if (!radii || !grad2d || !max_radii2D || !grad_accum || !denom)
      return set_error("densify stats: all five pointers or none"), 1;
    if (grad_stride < 2) return set_error("densify stats: grad_stride must be >= 2"), 1;
    a.radii = radii, a.grad2d = grad2d, a.gstride = grad_stride;
    a.max_r = max_radii2D, a.accum = grad_accum, a.denom = denom;
  }
  GeomPtrs geo;
  geom_layout((size_t)P, &geo, (char*)view->geom_buffer);
  a.err = &geo.counters[CNT_ERR];
  a.splat = geo.splat;  // (z of the depth chain)
  a.invdepth_sums = invdepth_sums;
  const CameraArgs c = make_camera(nullptr, view->image_width, view->image_height, view->viewmatrix, view->projmatrix,
                                   view->campos, view->tan_fovx, view->tan_fovy, 0);
  bwd_gaussians_adam(g, c, geo, a, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream) {
  clear_error(0);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (P > 0 && (!means3D || !viewmatrix || !present)) return set_error("missing pointer"), 1;
  mark_visible(P, means3D, viewmatrix, projmatrix, present, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

size_t gs_knn_scratch_bytes(int P) { return knn_scratch_bytes(P); }

int gs_knn_mean_dist2(int P, const float* points, float* out, void* scratch, void* stream) {
  clear_error(0);
  if (P < 0) return set_error("P must be >= 0"), 1;
  if (P == 0) return 0;
  if (!points || !out || !scratch) return set_error("missing pointer"), 1;
  knn_mean_dist2(P, points, out, (char*)scratch, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

unsigned gs_debug_set_scan_spin_limit(unsigned limit) {
  return gs::g_spin_limit.exchange(limit, std::memory_order_relaxed);
}

int gs_debug_set_tile_sort_packed(int on) {
  return gs::g_tile_sort_packed.exchange(on ? 1 : 0, std::memory_order_relaxed);
}
long long gs_debug_tile_sort_packed_count(void) { return gs::g_tile_sort_packed_n.load(std::memory_order_relaxed); }

int gs_debug_sh_rows_staged(int D, int M, const void* shs) { return gs::sh_rows_stageable(D, M, shs) ? 1 : 0; }

/* ---- launched-kernel log (tests: every kernel in the code object is launched by some test) ---- */
int gs_debug_launch_log(int enable) {
  const int prev = gs::launch_log_on();
  gs::g_launch_log.store(enable ? 1 : 0, std::memory_order_relaxed);
  return prev;
}

long long gs_debug_launched_kernels(char* buf, long long cap) {
  std::string out;
  {
    std::lock_guard<std::mutex> lk(gs::g_launch_mu);
    for (const void* k : gs::g_launched) {
      Dl_info info;
      if (dladdr(k, &info) && info.dli_sname && info.dli_saddr == k)
        out += info.dli_sname;
      else
        out += "?";
      out += '\n';
    }
  }
  if (buf && cap > (long long)out.size()) memcpy(buf, out.c_str(), out.size() + 1);
  return (long long)out.size();
}

/* ---- numerics mode of the render loops ---- */
int gs_set_exact_exp(int exact) {
  const int prev = exact_exp() ? 1 : 0;
  gs::g_exact_exp.store(exact ? 1 : 0, std::memory_order_relaxed);
  return prev;
}

/* ---- fused SSIM (utils/loss_utils.py:ssim) ---- */
size_t gs_ssim_partial_count(int planes, int H, int W) { return ssim_partial_count(planes, H, W); }

int gs_ssim_forward(int planes, int H, int W, const float* window11_host, const float* img1, const float* img2,
                    float* dmaps, float* partial, float* plane_sum, void* stream) {
  clear_error(0);
  if (planes <= 0 || H <= 0 || W <= 0) return set_error("ssim: empty image"), 1;
  if (!window11_host || !img1 || !img2 || !dmaps || !partial || !plane_sum) return set_error("ssim: missing pointer"), 1;
  ssim_forward(planes, H, W, window11_host, img1, img2, dmaps, partial, plane_sum, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_ssim_backward(int planes, int channels, int H, int W, const float* window11_host, const float* img1,
                     const float* img2, const float* dmaps, const float* scale, float* dimg1, void* stream) {
  clear_error(0);
  if (planes <= 0 || H <= 0 || W <= 0 || channels <= 0 || planes % channels) return set_error("ssim: bad shape"), 1;
  if (!window11_host || !img1 || !img2 || !dmaps || !scale || !dimg1) return set_error("ssim: missing pointer"), 1;
  ssim_backward(planes, channels, H, W, window11_host, img1, img2, dmaps, scale, dimg1, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

/* ---- skysphere background (GSRAST_HAS_SKY) ---- */
size_t gs_sky_scratch_bytes(int Hs, int Ws) { return Hs > 0 && Ws > 0 ? sky_scratch_bytes(Hs, Ws) : 0; }

static bool sky_shape_ok(int W, int H, int Hs, int Ws) {
  if (W < 1 || H < 1) return set_error("sky: image size must be positive (got %d x %d)", W, H), false;
  if (Hs < 1 || Ws < 1) return set_error("sky: texture size must be positive (got %d x %d)", Ws, Hs), false;
  if (Hs > SKY_MAX_TEX || Ws > SKY_MAX_TEX) return set_error("sky: texture side above %d texels", SKY_MAX_TEX), false;
  return true;
}

int gs_sky_compose_forward(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                           const float* texture, const float* color, const float* alpha, float* out_image,
                           void* stream) {
  clear_error(0);
  if (!sky_shape_ok(W, H, Hs, Ws)) return 1;
  if (!viewmatrix || !texture || !out_image) return set_error("sky: missing pointer"), 1;
  sky_forward(W, H, viewmatrix, tanfovx, tanfovy, Hs, Ws, texture, color, alpha, out_image, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_sky_compose_backward(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                            const float* texture, const float* alpha, const float* dL_dimage, float* dL_dalpha,
                            float* dL_dtexture, int accumulate_texture, void* scratch, void* stream) {
  clear_error(0);
  if (!sky_shape_ok(W, H, Hs, Ws)) return 1;
  if (!viewmatrix || !texture || !dL_dimage) return set_error("sky: missing pointer"), 1;
  if (dL_dtexture && !scratch) return set_error("sky: dL_dtexture needs the scratch of gs_sky_scratch_bytes"), 1;
  if (dL_dtexture && (((uintptr_t)scratch) & 15)) return set_error("sky: scratch must be 16-byte aligned"), 1;
  if (!dL_dalpha && !dL_dtexture) return 0;
  sky_backward(W, H, viewmatrix, tanfovx, tanfovy, Hs, Ws, texture, alpha, dL_dimage, dL_dalpha, dL_dtexture,
               accumulate_texture != 0, (char*)scratch, nullptr, false, nullptr, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

/* GSRAST_HAS_SKY_CAMERA */
size_t gs_sky_camera_scratch_bytes(int W, int H) { return W > 0 && H > 0 ? sky_camera_scratch_bytes(W, H) : 0; }

int gs_sky_compose_backward_camera(int W, int H, const float* viewmatrix, float tanfovx, float tanfovy, int Hs, int Ws,
                                   const float* texture, const float* alpha, const float* dL_dimage, float* dL_dalpha,
                                   float* dL_dtexture, int accumulate_texture, void* scratch, float* dL_dviewmatrix,
                                   int accumulate_view, void* camera_scratch, void* stream) {
  clear_error(0);
  if (!sky_shape_ok(W, H, Hs, Ws)) return 1;
  if (!viewmatrix || !texture || !dL_dimage) return set_error("sky: missing pointer"), 1;
  if (dL_dtexture && !scratch) return set_error("sky: dL_dtexture needs the scratch of gs_sky_scratch_bytes"), 1;
  if (dL_dtexture && (((uintptr_t)scratch) & 15)) return set_error("sky: scratch must be 16-byte aligned"), 1;
  if (dL_dviewmatrix && !camera_scratch)
    return set_error("sky: dL_dviewmatrix needs the scratch of gs_sky_camera_scratch_bytes"), 1;
  if (dL_dviewmatrix && (((uintptr_t)camera_scratch) & 15))
    return set_error("sky: camera_scratch must be 16-byte aligned"), 1;
  if (!dL_dalpha && !dL_dtexture && !dL_dviewmatrix) return 0;
  sky_backward(W, H, viewmatrix, tanfovx, tanfovy, Hs, Ws, texture, alpha, dL_dimage, dL_dalpha, dL_dtexture,
               accumulate_texture != 0, (char*)scratch, dL_dviewmatrix, accumulate_view != 0, (double*)camera_scratch,
               (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

/* ---- fused photometric loss (train.py:91-92) ---- */
int gs_photometric_loss_forward(int planes, int H, int W, const float* window11_host, const float* img,
                                const float* gt, float lambda_dssim, float* dmaps, float* partial, float* out3,
                                void* stream) {
  clear_error(0);
  if (planes <= 0 || H <= 0 || W <= 0) return set_error("photometric loss: empty image"), 1;
  if (!window11_host || !img || !gt || !dmaps || !partial || !out3)
    return set_error("photometric loss: missing pointer"), 1;
  photometric_forward(planes, H, W, window11_host, img, gt, lambda_dssim, dmaps, partial, out3, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_photometric_loss_backward(int planes, int H, int W, const float* window11_host, const float* img,
                                 const float* gt, const float* dmaps, float lambda_dssim, const float* grad,
                                 float* dimg, void* stream) {
  clear_error(0);
  if (planes <= 0 || H <= 0 || W <= 0) return set_error("photometric loss: empty image"), 1;
  if (!window11_host || !img || !gt || !dmaps || !grad || !dimg)
    return set_error("photometric loss: missing pointer"), 1;
  photometric_backward(planes, H, W, window11_host, img, gt, dmaps, lambda_dssim, grad, dimg, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

/* ---- fused optimizer step and densification statistics (train.py:114-124) ---- */
int gs_adam_step(int count, float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                 float* const* exp_avg_sq_host, const long long* numel_host, const double* lr_host,
                 const long long* step_host, const double* weight_decay_host, double beta1, double beta2, double eps,
                 int maximize, void* stream) {
  clear_error(0);
  if (count < 0) return set_error("adam: count must be >= 0"), 1;
  if (count == 0) return 0;
  if (!params_host || !grads_host || !exp_avg_host || !exp_avg_sq_host || !numel_host || !lr_host || !step_host)
    return set_error("adam: missing pointer"), 1;
  for (int k = 0; k < count; k++) {
    if (numel_host[k] > 0 && (!params_host[k] || !grads_host[k] || !exp_avg_host[k] || !exp_avg_sq_host[k]))
      return set_error("adam: missing tensor pointer"), 1;
    if (step_host[k] < 1) return set_error("adam: step must be >= 1"), 1;
  }
  adam_step(count, params_host, grads_host, exp_avg_host, exp_avg_sq_host, numel_host, lr_host, step_host,
            weight_decay_host, beta1, beta2, eps, maximize != 0, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_adam_step_activated(int count, float* const* params_host, const float* const* grad_src_host,
                           const int* grad_mode_host, int sh_coeffs, float* const* exp_avg_host,
                           float* const* exp_avg_sq_host, const long long* numel_host, const double* lr_host,
                           const long long* step_host, const double* weight_decay_host, double beta1, double beta2,
                           double eps, int maximize, void* stream) {
  clear_error(0);
  if (count < 0) return set_error("adam: count must be >= 0"), 1;
  if (count == 0) return 0;
  if (!params_host || !grad_src_host || !grad_mode_host || !exp_avg_host || !exp_avg_sq_host || !numel_host ||
      !lr_host || !step_host)
    return set_error("adam: missing pointer"), 1;
  for (int k = 0; k < count; k++) {
    const long long n = numel_host[k];
    const int md = grad_mode_host[k];
    if (md < AG_PLAIN || md > AG_NORMALIZE) return set_error("adam: unknown gradient mode %d", md), 1;
    if (n > 0 && (!params_host[k] || !grad_src_host[k] || !exp_avg_host[k] || !exp_avg_sq_host[k]))
      return set_error("adam: missing tensor pointer"), 1;
    if (step_host[k] < 1) return set_error("adam: step must be >= 1"), 1;
    if ((md == AG_SH_DC || md == AG_SH_REST) && sh_coeffs < 1) return set_error("adam: sh_coeffs must be >= 1"), 1;
    if (md == AG_SH_DC && n % 3) return set_error("adam: features_dc must have 3 floats per Gaussian"), 1;
    if (md == AG_SH_REST && (sh_coeffs < 2 ? n != 0 : n % (3LL * (sh_coeffs - 1))))
      return set_error("adam: features_rest must have 3 (sh_coeffs - 1) floats per Gaussian"), 1;
    if ((md == AG_SH_DC || md == AG_SH_REST) && n >= (1LL << 32)) return set_error("adam: SH tensor too large"), 1;
    if (md == AG_NORMALIZE && (n % 4 || ((uintptr_t)grad_src_host[k] & 15)))
      return set_error("adam: rotation rows of 4 floats with a 16-byte aligned gradient source required"), 1;
  }
  adam_step(count, params_host, grad_src_host, exp_avg_host, exp_avg_sq_host, numel_host, lr_host, step_host,
            weight_decay_host, beta1, beta2, eps, maximize != 0, (hipStream_t)stream, grad_mode_host, sh_coeffs);
  return t_failed ? 1 : 0;
}

int gs_activate_forward(int P, int sh_rest, const float* features_dc, const float* features_rest,
                        const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, float* shs,
                        float* opacity, float* scales, float* rotations, void* stream) {
  clear_error(0);
  if (P < 0 || sh_rest < 0) return set_error("activate: P and sh_rest must be >= 0"), 1;
  if (P == 0) return 0;
  // shs may be null: only opacity / scales / rotations are activated (split-SH rasterizer inputs)
  if ((shs && (!features_dc || (sh_rest && !features_rest))) || !opacity_raw || !scaling_raw || !rotation_raw ||
      !opacity || !scales || !rotations)
    return set_error("activate: missing pointer"), 1;
  if (((uintptr_t)rotation_raw | (uintptr_t)rotations | (uintptr_t)shs) & 15)
    return set_error("activate: rotation / shs buffers must be 16-byte aligned"), 1;
  activate_forward(P, sh_rest, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, shs, opacity,
                   scales, rotations, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_activate_backward(int P, int sh_rest, const float* dL_dshs, const float* dL_dopacity, const float* dL_dscales,
                         const float* dL_drotations, const float* opacity, const float* scales,
                         const float* rotation_raw, float* dL_dfeatures_dc, float* dL_dfeatures_rest,
                         float* dL_dopacity_raw, float* dL_dscaling_raw, float* dL_drotation_raw, void* stream) {
  clear_error(0);
  if (P < 0 || sh_rest < 0) return set_error("activate: P and sh_rest must be >= 0"), 1;
  if (P == 0) return 0;
  if ((dL_dshs && (!dL_dfeatures_dc || (sh_rest && !dL_dfeatures_rest))) ||
      (dL_dopacity && (!opacity || !dL_dopacity_raw)) || (dL_dscales && (!scales || !dL_dscaling_raw)) ||
      (dL_drotations && (!rotation_raw || !dL_drotation_raw)))
    return set_error("activate: missing pointer"), 1;
  if (((uintptr_t)dL_dshs | (uintptr_t)dL_drotations | (uintptr_t)rotation_raw | (uintptr_t)dL_drotation_raw) & 15)
    return set_error("activate: rotation / shs buffers must be 16-byte aligned"), 1;
  activate_backward(P, sh_rest, dL_dshs, dL_dopacity, dL_dscales, dL_drotations, opacity, scales, rotation_raw,
                    dL_dfeatures_dc, dL_dfeatures_rest, dL_dopacity_raw, dL_dscaling_raw, dL_drotation_raw,
                    (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

/* ---- densify_and_prune (gaussian_model.py:391-403) ---- */
static DensifyParams make_dens_params(double grad_threshold, double pd_extent, double min_opacity, double big_extent,
                                      int has_screen, double max_screen, int N) {
  DensifyParams dp;
  dp.thr = (float)grad_threshold;
  dp.pd_ext = (float)pd_extent;
  dp.min_op = (float)min_opacity;
  dp.big_ext = (float)big_extent;
  dp.max_screen = (float)max_screen;
  dp.inv_split = 1.0f / (float)(0.8 * N);
  dp.screen = has_screen ? 1 : 0;
  return dp;
}

size_t gs_densify_block_count(int P) { return P > 0 ? (size_t)((P + 255) / 256) : 0; }

int gs_densify_classify(int P, const float* grad_accum, const float* denom, const float* opacity_raw,
                        const float* scaling_raw, double grad_threshold, double pd_extent, double min_opacity,
                        double big_extent, int has_screen, double max_screen, int N, uint8_t* flags,
                        uint32_t* block_counts, uint32_t* totals, void* stream) {
  clear_error(0);
  if (P <= 0 || N < 1) return set_error("densify: P must be > 0 and N >= 1"), 1;
  if (!grad_accum || !denom || !opacity_raw || !scaling_raw || !flags || !block_counts || !totals)
    return set_error("densify: missing pointer"), 1;
  const DensifyParams dp = make_dens_params(grad_threshold, pd_extent, min_opacity, big_extent, has_screen,
                                            max_screen, N);
  densify_classify(P, dp, grad_accum, denom, opacity_raw, scaling_raw, flags, block_counts, totals,
                   (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_densify_split_stds(int P, int N, const uint32_t* totals_host, const uint8_t* flags,
                          const uint32_t* block_counts, const float* scaling_raw, float* stds, void* stream) {
  clear_error(0);
  if (P <= 0 || N < 1 || !totals_host) return set_error("densify: bad arguments"), 1;
  if (totals_host[2] == 0) return 0;
  if (!flags || !block_counts || !scaling_raw || !stds) return set_error("densify: missing pointer"), 1;
  densify_stds(P, N, totals_host[2], flags, block_counts, scaling_raw, stds, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_densify_emit(int P, int N, const uint32_t* totals_host, const uint8_t* flags, const uint32_t* block_counts,
                    const float* samples, const float* const* params_host, const float* const* exp_avg_host,
                    const float* const* exp_avg_sq_host, float* const* out_params_host,
                    float* const* out_exp_avg_host, float* const* out_exp_avg_sq_host, const int* widths_host,
                    void* stream) {
  clear_error(0);
  if (P <= 0 || N < 1 || !totals_host || !flags || !block_counts || !params_host || !out_params_host || !widths_host)
    return set_error("densify: missing argument"), 1;
  if (totals_host[2] && !samples) return set_error("densify: split samples missing"), 1;
  if (widths_host[DT_XYZ] != 3 || widths_host[DT_FDC] != 3 || widths_host[DT_OPACITY] != 1 ||
      widths_host[DT_SCALING] != 3 || widths_host[DT_ROT] != 4 || widths_host[DT_FREST] < 0)
    return set_error("densify: row widths must be xyz 3, f_dc 3, f_rest 3K, opacity 1, scaling 3, rotation 4"), 1;
  // P' == 0 (everything pruned): the outputs are zero-row tensors, whose data pointers may be NULL
  const bool rows = (uint64_t)totals_host[0] + totals_host[1] + (uint64_t)N * totals_host[3] != 0;
  DensTensors t;
  for (int q = 0; q < DENS_TENSORS; q++) {
    t.src[q] = params_host[q];
    t.dst[q] = out_params_host[q];
    t.width[q] = widths_host[q];
    const bool has_m = exp_avg_host && exp_avg_host[q];
    if (has_m && (!exp_avg_sq_host || !exp_avg_sq_host[q] ||
                  (rows && (!out_exp_avg_host || !out_exp_avg_host[q] || !out_exp_avg_sq_host ||
                            !out_exp_avg_sq_host[q]))))
      return set_error("densify: incomplete optimizer state pointers"), 1;
    t.m_src[q] = has_m ? exp_avg_host[q] : nullptr;
    t.v_src[q] = has_m ? exp_avg_sq_host[q] : nullptr;
    t.m_dst[q] = has_m && rows ? out_exp_avg_host[q] : nullptr;
    t.v_dst[q] = has_m && rows ? out_exp_avg_sq_host[q] : nullptr;
    if ((!t.src[q] || (rows && !t.dst[q])) && t.width[q] > 0)
      return set_error("densify: missing parameter pointer"), 1;
  }
  if (!rows) return 0;  // nothing to write: no launch
  DensCounts n{totals_host[0], totals_host[1], totals_host[2], totals_host[3]};
  const DensifyParams dp = make_dens_params(0, 0, 0, 0, 0, 0, N);
  densify_emit(P, N, dp, n, flags, block_counts, samples, t, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_densify_stats(int P, const int* radii, const float* grad2d, int grad_stride, float* max_radii2D,
                     float* grad_accum, float* denom, void* stream) {
  clear_error(0);
  if (P < 0) return set_error("densify_stats: P must be >= 0"), 1;
  if (P == 0) return 0;
  if (grad_stride < 2) return set_error("densify_stats: grad_stride must be >= 2"), 1;
  if (!radii || !grad2d || !max_radii2D || !grad_accum || !denom) return set_error("densify_stats: missing pointer"), 1;
  densify_stats(P, radii, grad2d, grad_stride, max_radii2D, grad_accum, denom, (hipStream_t)stream);
  return t_failed ? 1 : 0;
}

int gs_debug_export(int P, int W, int H, long long num_rendered, const void* geom_buffer, const void* binning_buffer,
                    const void* image_buffer, uint32_t* point_list, uint32_t* ranges, float* xy, float* conic_opacity,
                    float* rgb, float* depth, uint32_t* tiles_touched, float* final_T, uint32_t* n_contrib,
                    void* stream) {
  clear_error(0);
  hipStream_t st = (hipStream_t)stream;
  if (P <= 0) return 0;
  if (W <= 0 || H <= 0) return set_error("debug_export: image size must be positive (got %d x %d)", W, H), 1;
  if (size_limit_error(W, H, "debug_export: ")) return 1;
  const int gx = (W + GS_TILE - 1) / GS_TILE, gy = (H + GS_TILE - 1) / GS_TILE;
  const Layouts L(P, num_rendered, size_camera(W, H), geom_buffer, binning_buffer, image_buffer);
  if (point_list && num_rendered > 0)
    GS_LAUNCH("export_list", k_export_list, dim3((unsigned)((num_rendered + 255) / 256)), dim3(256), 0, st,
              (uint32_t)num_rendered, L.geo.counters, L.bin.point_list, L.bin.presort_gid, point_list);
  if (ranges)
    check_hip(hipMemcpyAsync(ranges, L.img.ranges, sizeof(uint2) * gx * gy, hipMemcpyDeviceToDevice, st), "copy");
  if (xy || conic_opacity || rgb || depth)
    GS_LAUNCH("export_splat", k_export_splat, dim3((P + 255) / 256), dim3(256), 0, st, P, L.geo.splat, xy,
              conic_opacity, rgb, depth);
  if (tiles_touched)
    check_hip(hipMemcpyAsync(tiles_touched, L.geo.tiles, sizeof(uint32_t) * P, hipMemcpyDeviceToDevice, st), "copy");
  if (final_T)
    check_hip(hipMemcpyAsync(final_T, L.img.final_T, sizeof(float) * W * H, hipMemcpyDeviceToDevice, st), "copy");
  if (n_contrib)
    check_hip(hipMemcpyAsync(n_contrib, L.img.n_contrib, sizeof(uint32_t) * W * H, hipMemcpyDeviceToDevice, st),
              "copy");
  return t_failed ? 1 : 0;
}

int gs_debug_export_slots(int W, int H, long long num_rendered, const void* binning_buffer, const void* image_buffer,
                          uint32_t* slots, uint32_t* tile_cut, void* stream) {
  clear_error(0);
  hipStream_t st = (hipStream_t)stream;
  if (W <= 0 || H <= 0 || num_rendered < 0) return set_error("debug_export_slots: bad arguments"), 1;
  if (size_limit_error(W, H, "debug_export_slots: ")) return 1;
  const int gx = (W + GS_TILE - 1) / GS_TILE, gy = (H + GS_TILE - 1) / GS_TILE;
  const Layouts L(0, num_rendered, size_camera(W, H), nullptr, binning_buffer, image_buffer);  // no geometry
  if (slots && num_rendered > 0)
    check_hip(hipMemcpyAsync(slots, L.bin.point_list, sizeof(uint32_t) * (size_t)num_rendered, hipMemcpyDeviceToDevice,
                             st), "copy");
  if (tile_cut)
    check_hip(hipMemcpyAsync(tile_cut, L.img.tile_cut, sizeof(uint32_t) * (size_t)gx * gy, hipMemcpyDeviceToDevice,
                             st), "copy");
  return t_failed ? 1 : 0;
}

void gs_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
}

int gs_profile_collect(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int n = 0;
  for (Pending& p : g_pending) {
    if (!p.b) continue;
    (void)hipEventSynchronize(p.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      bool found = false;
      for (ProfEntry& e : g_stats)
        if (e.name == p.name) {
          e.ms += ms;
          e.n += 1;
          found = true;
          break;
        }
      if (!found) g_stats.push_back(ProfEntry{p.name, (double)ms, 1});
      n++;
    }
    g_pool.push_back(p.a);
    g_pool.push_back(p.b);
  }
  g_pending.clear();
  return n;
}

void gs_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_stats.clear();
}

int gs_profile_stat(int i, char* name, int name_len, double* total_ms, long long* launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (i < 0 || i >= (int)g_stats.size()) return 0;
  if (name && name_len > 0) {
    strncpy(name, g_stats[i].name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (total_ms) *total_ms = g_stats[i].ms;
  if (launches) *launches = g_stats[i].n;
  return 1;
}

}  // extern "C"
