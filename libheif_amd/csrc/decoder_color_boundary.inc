// decoder_color_boundary.inc — part of decoder.hip (one translation unit: the parts share its file-local types and helpers), included from there.
// The colour boundary: device-resident planes, the planner (SURVEY a8), hipdec_color_convert and the image-level transforms.

// ---- colour boundary: device-resident planes, the planner (a8) and the image-level conversion ---------------------------
//
// libheif converts a decoded image through its own ColorConversionPipeline (libheif/color-conversion/colorconversion.cc:
// 279-623): a Dijkstra search over the registered ColorConversionOperations, then the chosen chain on host planes.  The
// integration op (libheif_amd/integration/colorconversion_hip.cc, registered in init_ops() with SpeedCosts_Hardware) hands
// the whole conversion to hipdec_color_convert(): the planner below restates the decisions of that search for the in-scope
// states (SURVEY.md §3.5), the fused HIP kernels of color.hip execute the chain, and when the input planes are the ones a
// hipdec decoder has just copied into libheif's image, the kernels read the DEVICE copy instead of uploading them again.
namespace {

struct ResidentPlane {
  const void* host = nullptr;      // where hipdec_decoder_read_plane_tracked() copied the plane
  size_t host_stride = 0;
  int w = 0, h = 0, bits = 0;
  uint64_t sample = 0;             // hash of the host copy at hand-over time: EVERY byte (plane_hash), or - mode 2 - every 16th row
  int mode = 1;                    // the tracking mode the hash was taken in
  std::shared_ptr<hipdec_batch> batch;   // a decoder's output plane: (batch, item, comp) ...
  int item = 0, comp = 0;
  std::shared_ptr<void> buffer;           // ... or a plane of a device buffer this entry keeps alive (transform result, grid canvas)
  const uint8_t* dev = nullptr;
  size_t dev_stride = 0;
  int device = 0;
  uint64_t tick = 0;
  std::chrono::steady_clock::time_point born{};
};
std::mutex g_res_mu;
// (heap-allocated and never destroyed: its entries own batches, and destroying those from a static destructor at process exit would
//  run after the HIP runtime and this library's pools are gone; hipdec_shutdown() / the plugin's deinit empty it in good time)
std::unordered_map<const void*, ResidentPlane>& g_resident = *new std::unordered_map<const void*, ResidentPlane>();   // by host plane address
uint64_t g_res_tick = 0;
std::atomic<uint64_t> g_cb_conversions{0}, g_cb_resident{0}, g_cb_launches{0}, g_xf_transforms{0}, g_grid_canvases{0}, g_img_scales{0};

// Content identity of a host plane: EVERY byte of every row (64-bit lanes, four independent multiply-rotate chains, ~10 GB/s on one
// host core).  libheif edits decoded planes in place between the plugin's hand-over and the colour conversion (mirror_inplace,
// image_item.cc:969: same pointer, stride and size), so a sampled hash is not an identity — round 2 sampled 16 rows x 96 bytes and could
// pair a mirrored luma plane with the un-mirrored device chroma when the samples happened to be symmetric (ADVICE round 2).
uint64_t plane_hash(const uint8_t* p, size_t stride, int w_bytes, int h)
{
  const uint64_t K1 = 0x9E3779B185EBCA87ull, K2 = 0xC2B2AE3D27D4EB4Full;
  uint64_t a = K1, b = K2, c = K1 ^ K2, d = ~K1;
  auto rot = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  for (int y = 0; y < h; y++) {
    const uint8_t* q = p + (size_t)y * stride;
    int i = 0;
    for (; i + 32 <= w_bytes; i += 32) {
      uint64_t w[4];
      memcpy(w, q + i, 32);
      a = rot(a ^ (w[0] * K2), 31) * K1; b = rot(b ^ (w[1] * K2), 29) * K1; c = rot(c ^ (w[2] * K2), 27) * K1; d = rot(d ^ (w[3] * K2), 33) * K1;
    }
    uint64_t tail[4] = {0, 0, 0, 0};
    if (i < w_bytes) {
      memcpy(tail, q + i, (size_t)(w_bytes - i));
      a = rot(a ^ (tail[0] * K2), 31) * K1; b = rot(b ^ (tail[1] * K2), 29) * K1; c = rot(c ^ (tail[2] * K2), 27) * K1; d = rot(d ^ (tail[3] * K2), 33) * K1;
    }
    a ^= (uint64_t)y * K2;   // the row index: swapped rows hash differently
  }
  uint64_t x = a ^ rot(b, 17) ^ rot(c, 33) ^ rot(d, 49);
  x ^= x >> 29; x *= K1; x ^= x >> 32;
  return x;
}

// The identity of tracking mode 2 (the host announces in-place edits through hipdec_forget_plane - the patched libheif of libheif_amd/integration
// does, its only in-place edit between hand-over and conversion being the mirror fall-back): the first and the last row and every 16th one.  Round 5
// measured the full hash at 38 ms per heif_decode_image() call under 256 threads (it reads 12 MB per 4K image twice, hand-over and conversion).
uint64_t plane_hash_mode(const uint8_t* p, size_t stride, int w_bytes, int h, int mode)
{
  if (mode != 2 || h <= 32) return plane_hash(p, stride, w_bytes, h);
  uint64_t x = plane_hash(p, stride * 16, w_bytes, (h + 15) / 16);
  return x ^ (plane_hash(p + (size_t)(h - 1) * stride, stride, w_bytes, 1) * 0x9E3779B185EBCA87ull);
}

// Tracking costs a pass over every decoded plane, so it only runs once a colour conversion has actually arrived at this library (the
// stock libheif never calls hipdec_color_convert: no hashing there); an entry serves ONE conversion and is dropped.  What the registry
// pins is bounded in TIME: libheif converts a decoded image within milliseconds of receiving its planes (same thread, same call), so an entry
// older than kResidentTtlMs (3 s) is stale - the host kept the planes without converting them - and goes at the next insert.  (Rounds 2 - 3 bounded it
// to 6 entries: with hundreds of application threads between read_plane and conversion the entries evicted each other and every conversion
// uploaded its planes again from pageable memory - 0.4 - 1.0 Gpixel/s of RGB through libheif where the planes alone ran at 3.)
// 0 off; 1 on, identity = a hash over every byte; 2 on for a host that ANNOUNCES its in-place edits (hipdec_forget_plane): identity = a hash over
// every 16th row - the safety net behind the announcements, not the identity itself
std::atomic<int> g_track_planes{getenv("HIPDEC_TRACK_PLANES") ? atoi(getenv("HIPDEC_TRACK_PLANES")) : 0};
const long kResidentTtlMs = getenv("HIPDEC_RESIDENT_TTL_MS") ? atol(getenv("HIPDEC_RESIDENT_TTL_MS")) : 3000;
constexpr size_t kMaxResident = 16384;

void resident_insert(struct ResidentPlane&& r);
}  // namespace
extern "C" void hipdec_forget_resident_planes(void);
namespace {

// Device rows -> a host buffer the caller owns (libheif's image planes: pageable memory).  A direct hipMemcpy2DAsync to pageable memory is
// staged by the runtime behind a process-wide lock at a few GB/s - with hundreds of application threads converting at once that was the whole
// drop-in RGB throughput (0.4 Gpixel/s at 1024 threads) - so the copy goes to pinned staging at link speed and the calling thread moves the rows
// itself (the threads do that in parallel).  Synchronises the stream.
// ... and it waits for its stream with a blocking event instead of hipStreamSynchronize's spin: the kernels of an image-level call queue up
// behind the resident CABAC pools of the decoder's launch sets (hundreds of ms under load), and a thousand application threads spinning
// through that starve the threads that feed the decoder (measured through libheif, 1024 threads x 4K stills to RGB: 0.36 Gpixel/s with
// launch sets of 10 stills).  (Admitting only a few callers at a time was tried and is worse - 0.17: each of them still waits for a
// pool to drain, so the waits have to overlap.)
hipError_t wait_stream_blocking(hipStream_t s)
{
  struct Ev { hipEvent_t e = nullptr; int device = -1; ~Ev() { if (e) (void)hipEventDestroy(e); } };
  static thread_local Ev ev;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (ev.e && ev.device != dev) { (void)hipEventDestroy(ev.e); ev.e = nullptr; }
  if (!ev.e) {
    if (hipEventCreateWithFlags(&ev.e, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev.e = nullptr; return hipStreamSynchronize(s); }
    ev.device = dev;
  }
  hipError_t e = hipEventRecord(ev.e, s);
  return e == hipSuccess ? hipEventSynchronize(ev.e) : e;
}

// HIPDEC_IMAGE_OPS_TIMING=1: where the host time of hipdec_color_convert goes, summed over all calls and printed at exit (development aid)
struct OpsTiming {
  std::atomic<uint64_t> calls{0}, find_us{0}, gpu_us{0}, copy_us{0}, hits{0}, misses{0};
  bool on = getenv("HIPDEC_IMAGE_OPS_TIMING") != nullptr;
  ~OpsTiming()
  {
    if (on && calls.load())
      fprintf(stderr, "[hipdec] color_convert: %llu calls; per call: locate planes %.2f ms (resident %llu, uploaded %llu), device work until synced %.2f ms, rows to the caller %.2f ms\n",
              (unsigned long long)calls.load(), find_us.load() / 1e3 / calls.load(), (unsigned long long)hits.load(), (unsigned long long)misses.load(),
              gpu_us.load() / 1e3 / calls.load(), copy_us.load() / 1e3 / calls.load());
  }
} g_ops_timing;
inline uint64_t us_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - t0).count(); }

int copy_rows_to_host(void* dst, size_t dst_stride, const void* dsrc, size_t src_stride, size_t row_bytes, int rows, hipStream_t s)
{
  void* pin = nullptr; size_t cap = 0;
  const size_t bytes = row_bytes * (size_t)rows;
  if (bytes >= (64u << 10) && pinned_acquire(&pin, bytes, &cap) == hipSuccess) {
    hipError_t e = hipMemcpy2DAsync(pin, row_bytes, dsrc, src_stride, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, s);
    const auto t_wait = Clock::now();
    if (e == hipSuccess) e = wait_stream_blocking(s);
    if (g_ops_timing.on) g_ops_timing.gpu_us += us_since(t_wait);
    if (e != hipSuccess) { pinned_release(pin, cap); return set_error(HIPDEC_ERR_DEVICE, "copy to host: %s", hipGetErrorString(e)); }
    const auto t_copy = Clock::now();
    if (dst_stride == row_bytes) memcpy(dst, pin, bytes);
    else for (int y = 0; y < rows; y++) memcpy((uint8_t*)dst + (size_t)y * dst_stride, (const uint8_t*)pin + (size_t)y * row_bytes, row_bytes);
    pinned_release(pin, cap);
    if (g_ops_timing.on) g_ops_timing.copy_us += us_since(t_copy);
    return 0;
  }
  (void)hipGetLastError();
  HIPDEC_CHECK_HIP(hipMemcpy2DAsync(dst, dst_stride, dsrc, src_stride, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, s));
  HIPDEC_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

void resident_note(hipdec_decoder* d, int c, const void* host, size_t stride)
{
  if (!g_track_planes.load(std::memory_order_relaxed)) return;
  hipdec_batch* pb = d->plane_batch();
  const int pitem = d->plane_item();
  const PicParams& P = pb->params[pitem];
  ResidentPlane r;
  r.host = host; r.host_stride = stride;
  r.w = c ? P.out_cwidth : P.out_width; r.h = c ? P.out_cheight : P.out_height;
  r.bits = c ? P.bit_depth_chroma : P.bit_depth_luma;
  r.mode = g_track_planes.load(std::memory_order_relaxed);
  r.sample = plane_hash_mode((const uint8_t*)host, stride, r.w * (pb->wide ? 2 : 1), r.h, r.mode);
  r.batch = d->out.batch ? d->out.batch : d->batch; r.item = pitem; r.comp = c;
  resident_insert(std::move(r));
}

// What an entry pins in HBM: a decoder's plane keeps the whole arena of its launch set alive, a buffer entry its transform result / grid canvas.
// Entries of one holder are counted once (the three planes of an image; up to 256 images of one launch set).
const void* resident_holder(const ResidentPlane& r) { return r.batch ? (const void*)r.batch.get() : (const void*)r.buffer.get(); }
size_t resident_holder_bytes(const ResidentPlane& r)
{
  if (r.batch) return r.batch->arena_capacity;
  return (size_t)r.dev_stride * (size_t)(r.h > 0 ? r.h : 1) * 2;   // (a canvas / transform result: its planes, roughly)
}
std::unordered_map<const void*, std::pair<int, size_t>>& g_res_holders = *new std::unordered_map<const void*, std::pair<int, size_t>>();
size_t g_res_bytes = 0;
uint64_t g_res_ops = 0;
// ADVICE round 4: the registry is bounded by what it PINS, not only by age - a host on the patched libheif that never converts colour never consumes
// entries.  Default: an eighth of the device's memory (HIPDEC_RESIDENT_MAX_BYTES overrides; 0 = no tracking at all).
size_t resident_byte_cap()
{
  static const size_t cap = [] {
    if (const char* e = getenv("HIPDEC_RESIDENT_MAX_BYTES")) return (size_t)strtoull(e, nullptr, 10);
    size_t free_b = 0, total = 0;
    if (hipMemGetInfo(&free_b, &total) != hipSuccess) { (void)hipGetLastError(); total = size_t(64) << 30; }
    return total / 8;
  }();
  return cap;
}
void resident_account(const ResidentPlane& r, int sign)   // g_res_mu held
{
  const void* h = resident_holder(r);
  if (!h) return;
  if (sign > 0) {
    auto& e = g_res_holders[h];
    if (e.first++ == 0) { e.second = resident_holder_bytes(r); g_res_bytes += e.second; }
  } else {
    auto it = g_res_holders.find(h);
    if (it != g_res_holders.end() && --it->second.first <= 0) { g_res_bytes -= std::min(g_res_bytes, it->second.second); g_res_holders.erase(it); }
  }
}
// g_res_mu held: entries older than the time to live, and - while the registry pins more than its byte cap or holds too many entries - the oldest ones
void resident_sweep(std::vector<ResidentPlane>& dropped, bool all_expired_only)
{
  const auto now = Clock::now();
  const auto limit = now - std::chrono::milliseconds(kResidentTtlMs);
  for (auto e = g_resident.begin(); e != g_resident.end();)
    if (e->second.born <= limit) { resident_account(e->second, -1); dropped.push_back(std::move(e->second)); e = g_resident.erase(e); } else ++e;
  if (all_expired_only) return;
  const size_t cap = resident_byte_cap();
  if (g_res_bytes <= cap && g_resident.size() < kMaxResident) return;
  std::vector<std::pair<uint64_t, const void*>> by_age;
  for (auto& e : g_resident) by_age.emplace_back(e.second.tick, e.first);
  std::sort(by_age.begin(), by_age.end());
  for (size_t i = 0; i < by_age.size() && (g_res_bytes > cap / 2 || g_resident.size() >= kMaxResident / 2); i++) {   // (down to half: not again at the next insert)
    auto it = g_resident.find(by_age[i].second);
    resident_account(it->second, -1);
    dropped.push_back(std::move(it->second));
    g_resident.erase(it);
  }
}

void resident_insert(ResidentPlane&& r)
{
  if (resident_byte_cap() == 0) return;
  static const bool hooked = [] { set_memory_pressure_handler(hipdec_forget_resident_planes); return true; }();   // a failing device allocation empties the registry
  (void)hooked;
  std::vector<ResidentPlane> dropped;   // what they keep alive dies outside the lock
  std::lock_guard<std::mutex> lock(g_res_mu);
  r.tick = ++g_res_tick;
  r.born = Clock::now();
  auto it = g_resident.find(r.host);
  if (it != g_resident.end()) { resident_account(it->second, -1); dropped.push_back(std::move(it->second)); g_resident.erase(it); }
  resident_account(r, +1);
  const void* key = r.host;
  g_resident.emplace(key, std::move(r));
  if ((++g_res_ops & 15u) == 0 || g_res_bytes > resident_byte_cap() || g_resident.size() >= kMaxResident) resident_sweep(dropped, false);
}

// a host plane that was just filled from a plane of `buffer` (w x h samples of `bits`, on the current device): a transform's result or the grid canvas
void resident_note_buffer(const void* host, size_t stride, int w, int h, int bits, const uint8_t* dev, size_t dev_stride, std::shared_ptr<void> buffer)
{
  if (!g_track_planes.load(std::memory_order_relaxed)) return;
  ResidentPlane r;
  r.host = host; r.host_stride = stride; r.w = w; r.h = h; r.bits = bits;
  r.mode = g_track_planes.load(std::memory_order_relaxed);
  r.sample = plane_hash_mode((const uint8_t*)host, stride, w * (bits > 8 ? 2 : 1), h, r.mode);
  r.buffer = std::move(buffer); r.dev = dev; r.dev_stride = dev_stride;
  (void)hipGetDevice(&r.device);
  resident_insert(std::move(r));
}

// device copy of a host plane handed over by a decoder of this library, if the host plane still holds exactly those bytes; the entry
// is consumed either way
bool resident_find(const void* host, size_t stride, int w, int h, int bits, const uint8_t** dev, size_t* dev_stride, std::shared_ptr<void>& keep,
                   hipdec_batch** from_batch = nullptr, int* from_item = nullptr)
{
  if (from_batch) *from_batch = nullptr;
  if (!g_track_planes.load(std::memory_order_relaxed)) g_track_planes.store(1, std::memory_order_relaxed);
  ResidentPlane r;
  {
    std::vector<ResidentPlane> dropped;
    std::unique_lock<std::mutex> lock(g_res_mu);
    if ((++g_res_ops & 15u) == 0) resident_sweep(dropped, true);   // (expired entries go from here too: a host that only converts still ages the registry)
    auto it = g_resident.find(host);
    const bool found = it != g_resident.end();
    if (found) { resident_account(it->second, -1); r = std::move(it->second); g_resident.erase(it); }
    lock.unlock();
    dropped.clear();
    if (!found) return false;
  }
  if (r.host_stride != stride || r.w != w || r.h != h || r.bits != bits) return false;
  if (r.batch && (r.batch->retired || !r.batch->arena)) return false;
  if (plane_hash_mode((const uint8_t*)host, stride, w * (bits > 8 ? 2 : 1), h, r.mode) != r.sample) return false;
  if (!r.batch) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != r.device) return false;
    *dev = r.dev; *dev_stride = r.dev_stride; keep = r.buffer;
    return true;
  }
  const PicParams& P = r.batch->params[r.item];
  *dev = r.batch->arena + P.off_out[r.comp];
  *dev_stride = P.out_stride[r.comp];
  keep = r.batch;
  if (from_batch) { *from_batch = r.batch.get(); if (from_item) *from_item = r.item; }
  return true;
}

}  // namespace

extern "C" {

void hipdec_set_plane_tracking(int on) { g_track_planes.store(on < 0 ? 0 : (on > 2 ? 2 : on), std::memory_order_relaxed); }

// the host is about to edit (or has freed) the plane at `host_plane`: its device copy must not serve a later conversion
void hipdec_forget_plane(const void* host_plane)
{
  ResidentPlane r;   // (dies outside the lock: an entry may own a batch)
  std::lock_guard<std::mutex> lock(g_res_mu);
  auto it = g_resident.find(host_plane);
  if (it == g_resident.end()) return;
  resident_account(it->second, -1);
  r = std::move(it->second);
  g_resident.erase(it);
}

void hipdec_forget_resident_planes(void)
{
  std::unordered_map<const void*, ResidentPlane> drop;
  {
    std::lock_guard<std::mutex> lock(g_res_mu);
    drop.swap(g_resident);
    g_res_holders.clear();
    g_res_bytes = 0;
  }
}   // the batches die here, outside the lock

void hipdec_resident_rgb_stats(uint64_t* images_produced, uint64_t* conversions_served)
{
  if (images_produced) *images_produced = g_rgb_produced.load();
  if (conversions_served) *conversions_served = g_rgb_served.load();
}

void hipdec_resident_plane_stats(uint64_t* entries, uint64_t* pinned_bytes)
{
  std::lock_guard<std::mutex> lock(g_res_mu);
  if (entries) *entries = g_resident.size();
  if (pinned_bytes) *pinned_bytes = g_res_bytes;
}

int hipdec_decoder_read_plane_tracked(hipdec_decoder* d, int c, void* dst, size_t dst_stride)
{
  int rc = hipdec_decoder_read_plane(d, c, dst, dst_stride);
  if (rc) return rc;
  return guarded("read_plane", [&]() -> int { resident_note(d, c, dst, dst_stride); return 0; });
}

void hipdec_color_boundary_stats(uint64_t* conversions, uint64_t* resident_planes, uint64_t* kernel_launches)
{
  if (conversions) *conversions = g_cb_conversions.load();
  if (resident_planes) *resident_planes = g_cb_resident.load();
  if (kernel_launches) *kernel_launches = g_cb_launches.load();
}

// a8 for the in-scope states: which chain ColorConversionPipeline::construct_pipeline (colorconversion.cc:279-435) ends up with.
// Every stock op costs SpeedCosts_Unoptimized, so the search returns the chain with the fewest steps; the rules below are the
// state_after_conversion() conditions of those ops (yuv2rgb.cc:35-92, :298-341, :430-478, :566-620; chroma_sampling.cc:501-560;
// hdr_sdr.cc:146-190; rgb2rgb.cc:30-70).  nclx "unspecified" (2) counts as the sRGB defaults for planning (nclx.cc:360-373).
int hipdec_color_plan(int bit_depth, int chroma, int has_alpha, const hipdec_nclx* nclx, int out_chroma, int upsampling, int only_preferred,
                      int ops[8], int* n_ops)
{
  if (!ops || !n_ops) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "color_plan: bad arguments");
  *n_ops = 0;
  int matrix = 6, full = 1;
  if (nclx && nclx->has_nclx) { matrix = nclx->matrix_coefficients == 2 ? 6 : nclx->matrix_coefficients; full = nclx->full_range_flag; }
  if (matrix == 11 || matrix == 14) return set_error(HIPDEC_ERR_UNSUPPORTED, "Unsupported color conversion (matrix_coefficients %d), as in the reference", matrix);
  if (chroma == 0) {   // heif_chroma_monochrome: Op_mono_to_RGB24_32 (8-bit; RGB24 only without an alpha plane)
    if (bit_depth != 8 || !(out_chroma == 11 || (out_chroma == 10 && !has_alpha)))
      return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: this monochrome conversion is left to the stock ops");
    ops[(*n_ops)++] = HIPDEC_OP_MONO_TO_RGB24_32;
    return 0;
  }
  if (chroma < 1 || chroma > 3) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: input chroma %d is outside the HEIC hot path", chroma);
  const bool nn_allowed = !(only_preferred && upsampling != 1);
  auto push = [&](int op) { ops[(*n_ops)++] = op; };
  if (out_chroma == 10 || out_chroma == 11) {          // interleaved RGB / RGBA, 8 bit
    if (out_chroma == 10 && has_alpha) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: dropping an alpha plane is left to the stock ops");
    if (bit_depth > 8) {
      // > 8-bit planes to 8-bit interleaved RGB: the search of the reference ends on one of two chains (checked state by state against the compiled
      // pipeline, tests/test_color_emu.py): Op_to_sdr_planes FIRST when the 8-bit chain behind it is shorter (the 4:2:0 integer op) or when the
      // preferred upsampling has to run anyway; otherwise the generic op at the input depth, THEN Op_to_sdr_planes on R, G, B
      if (has_alpha) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: > 8-bit planes with alpha to 8-bit RGB are left to the stock ops");
      const bool int_op = chroma == 1 && nn_allowed && full && matrix != 0 && matrix != 8;
      if (!int_op && !(chroma != 3 && !nn_allowed)) { push(HIPDEC_OP_YCBCR_TO_RGB); push(HIPDEC_OP_TO_SDR); push(HIPDEC_OP_RGB_TO_RGB24_32); return 0; }
      push(HIPDEC_OP_TO_SDR); bit_depth = 8;
    }
    if (chroma == 1 && nn_allowed && full && matrix != 0 && matrix != 8) { push(out_chroma == 10 ? HIPDEC_OP_420_TO_RGB24 : HIPDEC_OP_420_TO_RGB32); return 0; }
    if (chroma != 3 && !nn_allowed) {
      push(chroma == 1 ? HIPDEC_OP_BILINEAR_420_TO_444 : HIPDEC_OP_BILINEAR_422_TO_444);
    }
    push(HIPDEC_OP_YCBCR_TO_RGB); push(HIPDEC_OP_RGB_TO_RGB24_32);
    return 0;
  }
  if (out_chroma == 12 || out_chroma == 14) {          // RRGGBB big / little endian
    if (has_alpha) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: RRGGBB from an image with alpha is left to the stock ops");
    if (bit_depth <= 8) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: 8-bit to RRGGBB needs Op_to_hdr_planes, outside the hot path");
    if (chroma == 1 && nn_allowed && matrix != 0 && matrix != 8) { push(HIPDEC_OP_420_TO_RRGGBB); return 0; }
    // every other state: the generic float op on the 16-bit planes (after the preferred upsampling when nearest neighbour is ruled out), then the
    // interleave, then the swap for little endian
    if (chroma != 3 && !nn_allowed) push(chroma == 1 ? HIPDEC_OP_BILINEAR_420_TO_444 : HIPDEC_OP_BILINEAR_422_TO_444);
    push(HIPDEC_OP_YCBCR_TO_RGB); push(HIPDEC_OP_RGB_HDR_TO_RRGGBB_BE);
    if (out_chroma == 14) push(HIPDEC_OP_SWAP_ENDIANNESS);
    return 0;
  }
  return set_error(HIPDEC_ERR_UNSUPPORTED, "color_plan: output chroma %d is outside the HEIC hot path", out_chroma);
}

int hipdec_color_convert(const hipdec_color_image* in, const hipdec_nclx* nclx, int out_chroma, int upsampling, int only_preferred,
                         void* out, size_t out_stride, int out_on_device)
{
  if (!in || !out || in->width <= 0 || in->height <= 0 || !in->plane[0] || (in->chroma != 0 && (!in->plane[1] || !in->plane[2])))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "color_convert: bad arguments");
  if (int rc = ensure_init()) return rc;
  return guarded("color_convert", [&]() -> int {
    int ops[8], n_ops = 0;
    const bool has_alpha = in->plane[3] != nullptr;
    if (int rc = hipdec_color_plan(in->bit_depth, in->chroma, has_alpha, nclx, out_chroma, upsampling, only_preferred, ops, &n_ops)) return rc;
    const int w = in->width, h = in->height;
    const int cw = in->chroma == 3 ? w : (w + 1) / 2, ch = in->chroma == 1 ? (h + 1) / 2 : h;
    int bits = in->bit_depth;
    size_t es = bits > 8 ? 2 : 1;
    const size_t out_bpp = out_chroma == 10 ? 3 : (out_chroma == 11 ? 4 : 6);
    if ((out_chroma == 10 || out_chroma == 11 || out_chroma == 12 || out_chroma == 14) && out_stride < (size_t)w * out_bpp)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "color_convert: out_stride %zu is smaller than a row of %zu bytes", out_stride, (size_t)w * out_bpp);
    for (int c = 0; c < 4; c++)
      if (in->plane[c] && in->stride[c] < (size_t)((c == 0 || c == 3) ? w : cw) * es)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "color_convert: stride %zu of plane %d is smaller than its rows", in->stride[c], c);
    hipStream_t s = stream_acquire_priority();
    struct Release { hipStream_t s; std::vector<std::pair<void*, size_t>> bufs;
                     ~Release() { (void)hipStreamSynchronize(s); for (auto& b : bufs) arena_release(b.first, b.second); stream_release(s); } } rel{s, {}};
    auto scratch = [&](size_t bytes, uint8_t** p) -> int {
      void* d = nullptr; size_t cap = 0;
      HIPDEC_CHECK_HIP(arena_acquire(&d, bytes ? bytes : 256, &cap));
      rel.bufs.emplace_back(d, cap); *p = (uint8_t*)d;
      return 0;
    };
    // ---- the input planes on the device: the decoder's own copy when the host planes are still the ones it handed over
    const uint8_t* dp[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t ds[4] = {0, 0, 0, 0};
    std::shared_ptr<void> keep[4];
    const auto t_find = Clock::now();
    if (g_ops_timing.on) g_ops_timing.calls++;
    // 8-bit 4:2:0 planes to interleaved RGB24 in ONE op: what a launch set of the decoder path can produce beside the planes (resident RGB).  Asking
    // for it earns the credit that makes the next launch sets carry it.
    // (the planner lists Op_YCbCr_to_RGB + Op_RGB_to_RGB24_32 as two ops; they run as one pass here and in the fused kernel)
    const bool rgb24_single = out_chroma == 10 && !has_alpha && in->chroma == 1 && in->bit_depth == 8 && !out_on_device && !in->on_device &&
                              ((n_ops == 1 && ops[0] == HIPDEC_OP_420_TO_RGB24) ||
                               (n_ops == 2 && ops[0] == HIPDEC_OP_YCBCR_TO_RGB && ops[1] == HIPDEC_OP_RGB_TO_RGB24_32));
    if (rgb24_single) rgb_note_wanted();
    hipdec_batch* from_b[4] = {nullptr, nullptr, nullptr, nullptr};
    int from_i[4] = {-1, -1, -1, -1};
    for (int c = 0; c < 4; c++) {
      if (!in->plane[c]) continue;
      const int pw = (c == 0 || c == 3) ? w : cw, ph = (c == 0 || c == 3) ? h : ch;
      if (in->on_device) { dp[c] = (const uint8_t*)in->plane[c]; ds[c] = in->stride[c]; continue; }
      if (resident_find(in->plane[c], in->stride[c], pw, ph, bits, &dp[c], &ds[c], keep[c], &from_b[c], &from_i[c])) {
        g_cb_resident++; if (g_ops_timing.on) g_ops_timing.hits++;
        if (c == 2 && rgb24_single && from_b[0] && from_b[0] == from_b[1] && from_b[1] == from_b[2] && from_i[0] == from_i[1] && from_i[1] == from_i[2]) {
          // all three planes are the untouched output of one decoded picture (resident_find compared every byte's hash): if its launch set emitted
          // RGB24 with exactly this colour description and the op the planner chose, the rows are already in pinned host memory
          hipdec_batch* rb = from_b[0];
          const size_t item = (size_t)from_i[0];
          if (item < rb->host_items.size() && rb->host_items[item].rgb && item < rb->pics.size()) {
            const hipdec_image_info& I = rb->pics[item].info;
            const int m = I.matrix_coeffs == 2 ? 6 : I.matrix_coeffs;
            const bool fused_int = I.full_range_flag && m != 0 && m != 8;
            if (nclx && nclx->has_nclx && nclx->colour_primaries == I.colour_primaries && nclx->transfer_characteristics == I.transfer_characteristics &&
                nclx->matrix_coefficients == I.matrix_coeffs && nclx->full_range_flag == I.full_range_flag && fused_int == (ops[0] == HIPDEC_OP_420_TO_RGB24) &&
                rb->params[item].out_width == w && rb->params[item].out_height == h) {
              const auto t_copy = Clock::now();
              const uint8_t* src = rb->host_items[item].rgb;
              const size_t row = (size_t)w * 3;
              if (out_stride == row) memcpy(out, src, row * (size_t)h);
              else for (int y = 0; y < h; y++) memcpy((uint8_t*)out + (size_t)y * out_stride, src + (size_t)y * row, row);
              rb->rgb_consumed++;
              g_rgb_served++;
              g_cb_conversions++;
              if (g_ops_timing.on) { g_ops_timing.find_us += us_since(t_find); g_ops_timing.copy_us += us_since(t_copy); }
              return 0;
            }
          }
        }
        continue;
      }
      if (g_ops_timing.on) g_ops_timing.misses++;
      uint8_t* d = nullptr;
      const size_t st = ((size_t)pw * es + 255) & ~(size_t)255;
      if (int rc = scratch(st * ph, &d)) return rc;
      HIPDEC_CHECK_HIP(hipMemcpy2DAsync(d, st, in->plane[c], in->stride[c], (size_t)pw * es, ph, hipMemcpyHostToDevice, s));
      dp[c] = d; ds[c] = st;
    }
    if (g_ops_timing.on) g_ops_timing.find_us += us_since(t_find);
    // ---- the chain
    int chroma = in->chroma, k = 0;
    if (k < n_ops && ops[k] == HIPDEC_OP_TO_SDR) {                     // a14 on every plane
      for (int c = 0; c < 4; c++) {
        if (!dp[c]) continue;
        const int pw = (c == 0 || c == 3) ? w : cw, ph = (c == 0 || c == 3) ? h : ch;
        uint8_t* d = nullptr;
        const size_t st = ((size_t)pw + 255) & ~(size_t)255;
        if (int rc = scratch(st * ph, &d)) return rc;
        if (int rc = hipdec_color_to_sdr(dp[c], ds[c], pw, ph, bits, d, st, (void*)s)) return rc;
        g_cb_launches++;
        dp[c] = d; ds[c] = st;
      }
      bits = 8; es = 1; k++;
    }
    if (k < n_ops && ops[k] == HIPDEC_OP_BILINEAR_420_TO_444) {         // a13 on both chroma planes
      for (int c = 1; c < 3; c++) {
        uint8_t* d = nullptr;
        const size_t st = ((size_t)w * es + 255) & ~(size_t)255;
        if (int rc = scratch(st * h, &d)) return rc;
        if (int rc = hipdec_color_bilinear_420_to_444(dp[c], ds[c], w, h, bits, d, st, (void*)s)) return rc;
        g_cb_launches++;
        dp[c] = d; ds[c] = st;
      }
      chroma = 3; k++;
    }
    if (k < n_ops && ops[k] == HIPDEC_OP_BILINEAR_422_TO_444) {         // SURVEY 8 f4, on both chroma planes
      for (int c = 1; c < 3; c++) {
        uint8_t* d = nullptr;
        const size_t st = ((size_t)w * es + 255) & ~(size_t)255;
        if (int rc = scratch(st * h, &d)) return rc;
        if (int rc = hipdec_color_bilinear_422_to_444(dp[c], ds[c], w, h, bits, d, st, (void*)s)) return rc;
        g_cb_launches++;
        dp[c] = d; ds[c] = st;
      }
      chroma = 3; k++;
    }
    uint8_t* dout = (uint8_t*)out;
    size_t dout_stride = out_stride;
    if (!out_on_device) {
      dout_stride = ((size_t)w * out_bpp + 255) & ~(size_t)255;
      if (int rc = scratch(dout_stride * h, &dout)) return rc;
    }
    if (k >= n_ops) return set_error(HIPDEC_ERR_UNSUPPORTED, "color_convert: empty chain");
    // The pipeline attaches the ColorState's profile - unspecified values replaced with the sRGB defaults - to every intermediate image
    // (colorconversion.cc:475, nclx.cc:360-373): an op that is not the first of its chain reads THAT profile, not the input image's.  It matters
    // for images without (or with unspecified) matrix_coefficients: computed BT.601 coefficients instead of the rounded default constants
    hipdec_nclx later{1, 1, 13, 6, 1};
    if (nclx && nclx->has_nclx) {
      later = *nclx;
      if (later.colour_primaries == 2) later.colour_primaries = 1;
      if (later.transfer_characteristics == 2) later.transfer_characteristics = 13;
      if (later.matrix_coefficients == 2) later.matrix_coefficients = 6;
    }
    if (k > 0) nclx = &later;
    int rc = 0;
    switch (ops[k]) {
      case HIPDEC_OP_MONO_TO_RGB24_32:
        rc = hipdec_color_mono_to_rgb24(dp[0], ds[0], dp[3], ds[3], w, h, dout, dout_stride, out_chroma == 11, (void*)s); break;
      case HIPDEC_OP_420_TO_RGB24:
        rc = hipdec_color_420_to_rgb24(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, nclx, dout, dout_stride, 0, (void*)s); break;
      case HIPDEC_OP_420_TO_RGB32:
        rc = hipdec_color_420_to_rgba_alpha(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, nclx, dp[3], ds[3], 1, 1, dout, dout_stride, (void*)s); break;
      case HIPDEC_OP_YCBCR_TO_RGB:   // a10 + a11 as one pass
        if (k + 1 < n_ops && ops[k + 1] == HIPDEC_OP_TO_SDR)     // > 8-bit planes to 8-bit RGB(A): generic op at the input depth, to_sdr on R, G, B, interleave
          rc = hipdec_color_hdr_to_rgb24(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, bits, chroma, nclx, dout, dout_stride, out_chroma == 11, 0, (void*)s);
        else if (out_chroma == 12 || out_chroma == 14)
          rc = hipdec_color_ycbcr_to_rrggbb_float(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, bits, chroma, nclx, dout, dout_stride, out_chroma == 14, (void*)s);
        else if (out_chroma == 11) rc = hipdec_color_420_to_rgba_alpha(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, nclx, dp[3], ds[3], 0, chroma, dout, dout_stride, (void*)s);
        else rc = hipdec_color_ycbcr_to_rgb24_float(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, chroma, nclx, dout, dout_stride, 0, (void*)s);
        break;
      case HIPDEC_OP_420_TO_RRGGBB:
        rc = hipdec_color_420_to_rrggbb(dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, bits, nclx, dout, dout_stride, out_chroma == 14, (void*)s); break;
      default: rc = set_error(HIPDEC_ERR_UNSUPPORTED, "color_convert: unplanned op %d", ops[k]); break;
    }
    if (rc) return rc;
    g_cb_launches++;
    if (!out_on_device) { if (int rc2 = copy_rows_to_host(out, out_stride, dout, dout_stride, (size_t)w * out_bpp, h, s)) return rc2; }
    else HIPDEC_CHECK_HIP(hipStreamSynchronize(s));
    g_cb_conversions++;
    return 0;
  });
}

// 'irot' / 'imir' / 'clap' of ImageItem::decode_image (libheif/image-items/image_item.cc:949-1081) over the planes of an image, on the device
// (plane kernels: transform.hip).  op HIPDEC_XF_ROTATE_CCW: args[0] = 90 / 180 / 270 (HeifPixelImage::rotate_ccw, image/pixelimage.cc:1175-1300);
// HIPDEC_XF_MIRROR: args[0] = heif_transform_mirror_direction (mirror_inplace, :1358-1430); HIPDEC_XF_CROP: args = left, right, top, bottom, the
// inclusive end points HeifPixelImage::crop takes (:1433-1530).  Where the reference first converts a subsampled image to 4:4:4 (odd sizes /
// offsets, the checks at :1187-1204, :1371-1381, :1457-1464) this returns HIPDEC_ERR_UNSUPPORTED and the caller keeps the host path.  The input
// planes are host or device pointers (host planes the decoder handed over are found device-resident); `out` brings the destination planes
// (NULL where the input has none) and receives the geometry.
int hipdec_image_transform(const hipdec_color_image* in, int op, const int* args, hipdec_color_image* out)
{
  if (!in || !out || !args || in->width <= 0 || in->height <= 0 || !in->plane[0] || in->bit_depth < 8 || in->bit_depth > 16)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: bad arguments");
  if (int rc = ensure_init()) return rc;
  return guarded("image_transform", [&]() -> int {
    const int w = in->width, h = in->height;
    const bool has_chroma = in->plane[1] && in->plane[2];
    const int chroma = has_chroma ? in->chroma : 0;
    if (has_chroma && (chroma < 1 || chroma > 3)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: chroma must be 1 (4:2:0), 2 (4:2:2) or 3 (4:4:4)");
    const bool odd_w = w & 1, odd_h = h & 1;
    int ow = w, oh = h, left = 0, top = 0;
    bool needs_444 = false;
    if (op == HIPDEC_XF_ROTATE_CCW) {
      const int a = args[0];
      if (a != 90 && a != 180 && a != 270) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: rotation must be 90, 180 or 270");
      if (chroma == 2) needs_444 = a != 180 || odd_h;
      else if (chroma == 1) needs_444 = (a == 90 && odd_w) || (a == 180 && (odd_w || odd_h)) || (a == 270 && odd_h);
      if (a != 180) { ow = h; oh = w; }
    } else if (op == HIPDEC_XF_MIRROR) {
      if (args[0] != 0 && args[0] != 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: mirror direction must be 0 or 1");
      if (chroma == 2) needs_444 = args[0] == 1 && odd_w;
      else if (chroma == 1) needs_444 = odd_w || odd_h;
    } else if (op == HIPDEC_XF_CROP) {
      const int l = args[0], r = args[1], t = args[2], b = args[3];
      if (l < 0 || t < 0 || r < l || b < t || r >= w || b >= h) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: invalid crop region");
      left = l; top = t; ow = r - l + 1; oh = b - t + 1;
      if (chroma == 2) needs_444 = l & 1;
      else if (chroma == 1) needs_444 = (l & 1) || (t & 1);
      // An odd window size leaves a half-covered chroma column / row at the edge.  The reference's output there is NOT the plane copy its
      // crop() reads like (measured through heif_decode_image on the compiled reference: the last chroma column / row differs from the
      // decoded plane), so those windows stay on the host rather than being claimed.
      if (!needs_444 && ((chroma == 1 || chroma == 2) && (ow & 1))) needs_444 = true;
      if (!needs_444 && chroma == 1 && (oh & 1)) needs_444 = true;
    } else return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: unknown operation %d", op);
    if (needs_444) return set_error(HIPDEC_ERR_UNSUPPORTED, "image_transform: odd size / offset of a subsampled image (the reference converts to 4:4:4 first or treats the half-covered chroma edge itself): host path");
    const size_t es = in->bit_depth > 8 ? 2 : 1;
    const int sx = (chroma == 1 || chroma == 2) ? 2 : 1, sy = chroma == 1 ? 2 : 1;
    hipStream_t s = stream_acquire_priority();
    struct Release { hipStream_t s; std::vector<std::pair<void*, size_t>> bufs;
                     ~Release() { (void)hipStreamSynchronize(s); for (auto& b : bufs) arena_release(b.first, b.second); stream_release(s); } } rel{s, {}};
    auto scratch = [&](size_t bytes, uint8_t** p) -> int {
      void* d = nullptr; size_t cap = 0;
      HIPDEC_CHECK_HIP(arena_acquire(&d, bytes ? bytes : 256, &cap));
      rel.bufs.emplace_back(d, cap); *p = (uint8_t*)d;
      return 0;
    };
    std::shared_ptr<void> keep[4];
    struct Result { int c, w, h; const uint8_t* dev; size_t dev_stride; std::shared_ptr<void> owner; };
    std::vector<Result> results;
    for (int c = 0; c < 4; c++) {
      if (!in->plane[c]) continue;
      if ((c == 1 || c == 2) && !has_chroma) continue;
      if (!out->plane[c]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: no destination for plane %d", c);
      const bool sub = c == 1 || c == 2;
      const int pw = sub ? (w + sx - 1) / sx : w, ph = sub ? (h + sy - 1) / sy : h;
      // geometry of this plane's result (crop: HeifPixelImage::crop's plane_left .. plane_right, pixelimage.cc:1497-1500)
      int pl = left, pt = top, pow_ = ow, poh = oh;
      if (sub) {
        if (op == HIPDEC_XF_CROP) { pl = left / sx; pt = top / sy; pow_ = (left + ow - 1) / sx - pl + 1; poh = (top + oh - 1) / sy - pt + 1; }
        else if (op == HIPDEC_XF_ROTATE_CCW && args[0] != 180) { pow_ = ph; poh = pw; }
        else { pow_ = pw; poh = ph; }
      }
      if (out->stride[c] < (size_t)pow_ * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_transform: destination stride of plane %d too small", c);
      const uint8_t* dp = nullptr; size_t ds = 0;
      if (in->on_device) { dp = (const uint8_t*)in->plane[c]; ds = in->stride[c]; }
      else if (resident_find(in->plane[c], in->stride[c], pw, ph, in->bit_depth, &dp, &ds, keep[c])) g_cb_resident++;
      else {
        uint8_t* d = nullptr;
        const size_t st = ((size_t)pw * es + 255) & ~(size_t)255;
        if (int rc = scratch(st * ph, &d)) return rc;
        HIPDEC_CHECK_HIP(hipMemcpy2DAsync(d, st, in->plane[c], in->stride[c], (size_t)pw * es, ph, hipMemcpyHostToDevice, s));
        dp = d; ds = st;
      }
      uint8_t* dout = (uint8_t*)out->plane[c];
      size_t dout_stride = out->stride[c];
      if (!out->on_device) {
        dout_stride = ((size_t)pow_ * es + 255) & ~(size_t)255;
        if (g_track_planes.load(std::memory_order_relaxed)) {
          // the result stays on the device behind its host copy: the next transform or the colour conversion of this image reads it there
          void* d = nullptr; size_t cap = 0;
          HIPDEC_CHECK_HIP(arena_acquire(&d, dout_stride * poh ? dout_stride * poh : 256, &cap));
          int dev_index = 0;
          (void)hipGetDevice(&dev_index);
          std::shared_ptr<void> owner(d, [cap, dev_index](void* q) { DeviceScope scope(dev_index); arena_release(q, cap); });
          dout = (uint8_t*)d;
          results.push_back(Result{c, pow_, poh, dout, dout_stride, std::move(owner)});
        } else if (int rc = scratch(dout_stride * poh, &dout)) return rc;
      }
      int rc;
      if (op == HIPDEC_XF_ROTATE_CCW) rc = hipdec_plane_rotate_ccw(dp, ds, pw, ph, (int)es, args[0], dout, dout_stride, (void*)s);
      else if (op == HIPDEC_XF_MIRROR) rc = hipdec_plane_mirror(dp, ds, pw, ph, (int)es, args[0], dout, dout_stride, (void*)s);
      else rc = hipdec_plane_crop(dp, ds, pw, ph, (int)es, pl, pt, pow_, poh, dout, dout_stride, (void*)s);
      if (rc) return rc;
      if (!out->on_device) { if (int rc2 = copy_rows_to_host((void*)out->plane[c], out->stride[c], dout, dout_stride, (size_t)pow_ * es, poh, s)) return rc2; }
    }
    HIPDEC_CHECK_HIP(hipStreamSynchronize(s));
    for (auto& r : results) resident_note_buffer(out->plane[r.c], out->stride[r.c], r.w, r.h, in->bit_depth, r.dev, r.dev_stride, std::move(r.owner));
    out->width = ow; out->height = oh; out->chroma = in->chroma; out->bit_depth = in->bit_depth;
    g_xf_transforms++;
    return 0;
  });
}

// heif_image_scale_image() (libheif/api/libheif/heif_image.cc:240 -> HeifPixelImage::scale_nearest_neighbor, image/pixelimage.cc:1783-1972) over the planes
// of an image, on the device: all planes as ONE launch of the plane scaler (color.hip).  HIPDEC_SCALE_NEAREST is the reference's arithmetic (every plane
// indexed with the IMAGE's sizes, chroma planes at the subsampled size of the output image), HIPDEC_SCALE_BOX the area average of heif_hipdec.h (every
// plane with its own sizes).  Same plane conventions as hipdec_image_transform.
int hipdec_image_scale(const hipdec_color_image* in, int out_width, int out_height, int filter, hipdec_color_image* out)
{
  if (!in || !out || in->width <= 0 || in->height <= 0 || !in->plane[0] || in->bit_depth < 8 || in->bit_depth > 16)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: bad arguments");
  if (out_width < 1 || out_height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: output size %d x %d", out_width, out_height);
  if (filter != HIPDEC_SCALE_NEAREST && filter != HIPDEC_SCALE_BOX) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: unknown filter %d", filter);
  if (int rc = ensure_init()) return rc;
  return guarded("image_scale", [&]() -> int {
    const int w = in->width, h = in->height;
    const bool has_chroma = in->plane[1] && in->plane[2];
    const int chroma = has_chroma ? in->chroma : 0;
    if (has_chroma && (chroma < 1 || chroma > 3)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: chroma must be 1 (4:2:0), 2 (4:2:2) or 3 (4:4:4)");
    const size_t es = in->bit_depth > 8 ? 2 : 1;
    const int sx = (chroma == 1 || chroma == 2) ? 2 : 1, sy = chroma == 1 ? 2 : 1;
    hipStream_t s = stream_acquire_priority();
    struct Release { hipStream_t s; std::vector<std::pair<void*, size_t>> bufs;
                     ~Release() { (void)hipStreamSynchronize(s); for (auto& b : bufs) arena_release(b.first, b.second); stream_release(s); } } rel{s, {}};
    auto scratch = [&](size_t bytes, uint8_t** p) -> int {
      void* d = nullptr; size_t cap = 0;
      HIPDEC_CHECK_HIP(arena_acquire(&d, bytes ? bytes : 256, &cap));
      rel.bufs.emplace_back(d, cap); *p = (uint8_t*)d;
      return 0;
    };
    std::shared_ptr<void> keep[4];
    struct Result { int c, w, h; const uint8_t* dev; size_t dev_stride; std::shared_ptr<void> owner; };
    std::vector<Result> results;
    PlaneScaleParams jobs[4];
    int job_plane[4], n_jobs = 0;
    for (int c = 0; c < 4; c++) {
      if (!in->plane[c]) continue;
      if ((c == 1 || c == 2) && !has_chroma) continue;
      if (!out->plane[c]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: no destination for plane %d", c);
      const bool sub = c == 1 || c == 2;
      const int pw = sub ? (w + sx - 1) / sx : w, ph = sub ? (h + sy - 1) / sy : h;
      const int qw = sub ? (out_width + sx - 1) / sx : out_width, qh = sub ? (out_height + sy - 1) / sy : out_height;   // get_subsampled_size, pixelimage.cc:1832-1843
      if (in->stride[c] < (size_t)pw * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: stride %zu of plane %d is smaller than its rows", in->stride[c], c);
      if (out->stride[c] < (size_t)qw * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_scale: destination stride of plane %d too small", c);
      const uint8_t* dp = nullptr; size_t ds = 0;
      if (in->on_device) { dp = (const uint8_t*)in->plane[c]; ds = in->stride[c]; }
      else if (resident_find(in->plane[c], in->stride[c], pw, ph, in->bit_depth, &dp, &ds, keep[c])) g_cb_resident++;
      else {
        uint8_t* d = nullptr;
        const size_t st = ((size_t)pw * es + 255) & ~(size_t)255;
        if (int rc = scratch(st * ph, &d)) return rc;
        HIPDEC_CHECK_HIP(hipMemcpy2DAsync(d, st, in->plane[c], in->stride[c], (size_t)pw * es, ph, hipMemcpyHostToDevice, s));
        dp = d; ds = st;
      }
      uint8_t* dout = (uint8_t*)out->plane[c];
      size_t dout_stride = out->stride[c];
      if (!out->on_device) {
        dout_stride = ((size_t)qw * es + 255) & ~(size_t)255;
        if (g_track_planes.load(std::memory_order_relaxed)) {
          // the result stays on the device behind its host copy: the colour conversion of the scaled image reads it there
          void* d = nullptr; size_t cap = 0;
          HIPDEC_CHECK_HIP(arena_acquire(&d, dout_stride * qh ? dout_stride * qh : 256, &cap));
          int dev_index = 0;
          (void)hipGetDevice(&dev_index);
          std::shared_ptr<void> owner(d, [cap, dev_index](void* q) { DeviceScope scope(dev_index); arena_release(q, cap); });
          dout = (uint8_t*)d;
          results.push_back(Result{c, qw, qh, dout, dout_stride, std::move(owner)});
        } else if (int rc = scratch(dout_stride * qh, &dout)) return rc;
      }
      jobs[n_jobs] = PlaneScaleParams{dp, ds, pw, ph, dout, dout_stride, qw, qh, w, h, out_width, out_height, 0};
      job_plane[n_jobs++] = c;
    }
    uint8_t* dev_params = nullptr;
    if (int rc = scratch(sizeof(jobs), &dev_params)) return rc;
    if (int rc = scale_planes_launch(jobs, n_jobs, (int)es, filter, dev_params, s)) return rc;
    if (!out->on_device)
      for (int k = 0; k < n_jobs; k++) {
        const int c = job_plane[k];
        if (int rc = copy_rows_to_host((void*)out->plane[c], out->stride[c], jobs[k].out, jobs[k].os, (size_t)jobs[k].qw * es, jobs[k].qh, s)) return rc;
      }
    HIPDEC_CHECK_HIP(hipStreamSynchronize(s));
    for (auto& r : results) resident_note_buffer(out->plane[r.c], out->stride[r.c], r.w, r.h, in->bit_depth, r.dev, r.dev_stride, std::move(r.owner));
    out->width = out_width; out->height = out_height; out->chroma = in->chroma; out->bit_depth = in->bit_depth;
    g_img_scales++;
    return 0;
  });
}

void hipdec_image_scale_stats(uint64_t* images) { if (images) *images = g_img_scales.load(); }

// hipdec_batch_to_tensor's single-image form: the planes of any image (found device-resident like hipdec_image_scale's, uploaded otherwise), the planner
// rules of hipdec_color_convert with nearest-neighbour chroma, all entries as ONE launch of the tensor kernel (color.hip).  plane[3] is ignored.
int hipdec_image_to_tensor(const hipdec_color_image* in, const hipdec_nclx* nclx, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, int n_entries,
                           void* out, size_t out_bytes, int out_on_device)
{
  if (!in || !out || in->width <= 0 || in->height <= 0 || !in->plane[0] || in->bit_depth < 8 || in->bit_depth > 14 || in->chroma < 0 || in->chroma > 3 ||
      (in->chroma != 0 && (!in->plane[1] || !in->plane[2])))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_to_tensor: bad arguments");
  size_t bytes = 0;
  if (int rc = tensor_check_desc("image_to_tensor", desc, n_entries, &bytes)) return rc;
  if (!entries && n_entries != 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_to_tensor: %d entries without an entry list (an image is one item)", n_entries);
  if (out_bytes < bytes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_to_tensor: out_bytes %zu is smaller than the tensor of %zu bytes", out_bytes, bytes);
  const int w = in->width, h = in->height, chroma = in->chroma;
  const size_t es = in->bit_depth > 8 ? 2 : 1;
  const int cw = chroma == 3 ? w : (w + 1) / 2, ch = chroma == 1 ? (h + 1) / 2 : h;
  for (int c = 0; c < (chroma ? 3 : 1); c++)
    if (in->stride[c] < (size_t)(c ? cw : w) * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "image_to_tensor: stride %zu of plane %d is smaller than its rows", in->stride[c], c);
  {
    int left, top, rw, rh;
    for (int e = 0; entries && e < n_entries; e++)
      if (int rc = tensor_window("image_to_tensor", entries + e, e, w, h, &left, &top, &rw, &rh)) return rc;
  }
  if (int rc = tensor_check_resample_depth("image_to_tensor", desc, in->bit_depth)) return rc;
  if (int rc = ensure_init()) return rc;
  return guarded("image_to_tensor", [&]() -> int {
    hipStream_t s = stream_acquire_priority();
    ColorBatchState blocks;
    struct Release { hipStream_t s; ColorBatchState& blocks; std::vector<std::pair<void*, size_t>> bufs;
                     ~Release() { (void)hipStreamSynchronize(s); color_batch_state_free(blocks); for (auto& b : bufs) arena_release(b.first, b.second); stream_release(s); } } rel{s, blocks, {}};
    auto scratch = [&](size_t n, uint8_t** p) -> int {
      void* d = nullptr; size_t cap = 0;
      HIPDEC_CHECK_HIP(arena_acquire(&d, n ? n : 256, &cap));
      rel.bufs.emplace_back(d, cap); *p = (uint8_t*)d;
      return 0;
    };
    const uint8_t* dp[3] = {nullptr, nullptr, nullptr};
    size_t ds[3] = {0, 0, 0};
    std::shared_ptr<void> keep[3];
    for (int c = 0; c < (chroma ? 3 : 1); c++) {
      const int pw = c ? cw : w, ph = c ? ch : h;
      if (in->on_device) { dp[c] = (const uint8_t*)in->plane[c]; ds[c] = in->stride[c]; continue; }
      if (resident_find(in->plane[c], in->stride[c], pw, ph, in->bit_depth, &dp[c], &ds[c], keep[c])) { g_cb_resident++; continue; }
      uint8_t* d = nullptr;
      const size_t st = ((size_t)pw * es + 255) & ~(size_t)255;
      if (int rc = scratch(st * ph, &d)) return rc;
      HIPDEC_CHECK_HIP(hipMemcpy2DAsync(d, st, in->plane[c], in->stride[c], (size_t)pw * es, ph, hipMemcpyHostToDevice, s));
      dp[c] = d; ds[c] = st;
    }
    if (!chroma) { dp[1] = dp[2] = dp[0]; ds[1] = ds[2] = ds[0]; }   // (never read)
    uint8_t* dout = (uint8_t*)out;
    if (!out_on_device) { if (int rc = scratch(bytes, &dout)) return rc; }
    // an op behind Op_to_sdr_planes reads the profile the pipeline attached to the intermediate image (see hipdec_color_convert)
    hipdec_nclx later{1, 1, 13, 6, 1};
    if (nclx && nclx->has_nclx) {
      later = *nclx;
      if (later.colour_primaries == 2) later.colour_primaries = 1;
      if (later.transfer_characteristics == 2) later.transfer_characteristics = 13;
      if (later.matrix_coefficients == 2) later.matrix_coefficients = 6;
    }
    const size_t entry_bytes = bytes / (size_t)n_entries;
    color_tensor_begin();
    for (int e = 0; e < n_entries; e++) {
      int left, top, rw, rh;
      int rc = tensor_window("image_to_tensor", entries ? entries + e : nullptr, e, w, h, &left, &top, &rw, &rh);
      if (!rc) rc = tensor_record_entry("image_to_tensor", dp[0], ds[0], dp[1], ds[1], dp[2], ds[2], w, h, in->bit_depth, chroma, nclx, &later, desc, left, top, rw, rh,
                                        entries ? entries[e].flip : 0, dout + (size_t)e * entry_bytes);
      if (rc) { color_tensor_abort(); return rc; }
    }
    if (int rc = color_tensor_launch(blocks, desc->filter, desc->dtype, s)) return rc;
    g_cb_launches++;
    if (!out_on_device) { if (int rc = copy_rows_to_host(out, bytes, dout, bytes, bytes, 1, s)) return rc; }
    else HIPDEC_CHECK_HIP(hipStreamSynchronize(s));
    g_tensor_calls++; g_tensor_entries += (uint64_t)n_entries;
    return 0;
  });
}

}  // extern "C"

