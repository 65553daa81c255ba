// decoder.hip — host orchestration of the decode pipeline and the hipdec_decoder_* / hipdec_batch_*
// entry points of the C ABI (include/heif_hipdec.h).
//
// hipdec_decoder mirrors the life cycle libheif drives through heif_decoder_plugin
// (libheif/codecs/decoder.cc:355-563; reference implementation libheif/plugins/decoder_libde265.cc);
// hipdec_batch is the device-side form of libheif's per-tile fan-out
// (libheif/image-items/grid.cc:405-453): all items of a grid / batch are parsed on the host, uploaded
// with ONE copy and decoded by ONE set of kernel launches, every CABAC substream and every CTB row
// of every item being an independent unit of GPU work.
#include "hipdec_internal.h"
#include "hevc_headers.h"
#include "kernels.h"
#include "batch_layout.h"
#include "color_device.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <unordered_map>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>


using namespace hipdec;

constexpr int kEv = 8;   // events per timing slot: start, parse, residual, recon, deblock, sao | colour begin, colour end

// resident-RGB policy: conversions that could have been served from a launch set's RGB earn credit, RGB that nobody fetched spends it
namespace { std::atomic<int> g_rgb_credit{0}; }
static void rgb_note_unused(int n) { if (n > 0) { int c = g_rgb_credit.load(); while (c > 0 && !g_rgb_credit.compare_exchange_weak(c, std::max(0, c - n))) {} } }
static void rgb_note_wanted() { int c = g_rgb_credit.load(); while (c < 4096 && !g_rgb_credit.compare_exchange_weak(c, std::min(4096, c + 64))) {} }
static bool rgb_wanted() { static const bool off = getenv("HIPDEC_NO_RESIDENT_RGB") != nullptr; return !off && g_rgb_credit.load(std::memory_order_relaxed) > 0; }

struct hipdec_batch : BatchLayout {
  int device = 0;               // the device the arena lives on: every entry point that touches the batch runs under its scope
  uint8_t* arena = nullptr;
  size_t arena_capacity = 0;
  void* staging = nullptr;      // pinned upload staging (large batches), returned to its pool once the upload has completed
  size_t staging_capacity = 0;
  void* upload_dev = nullptr;   // a batch that takes over a busy arena: its upload region lands here first (beside the predecessor's kernels), build_batch
  size_t upload_dev_capacity = 0;
  hipEvent_t uploaded = nullptr;   // recorded on the upload stream behind the H2D copy; launch streams wait on it
  hipEvent_t done = nullptr;       // recorded behind the last piece of work enqueued for this batch (decode, colour stage, packs)
  bool done_recorded = false;
  int32_t* host_status = nullptr;  // pinned: the device status word of the last run, copied behind its kernels (the arena may already
                                   // belong to the next batch when hipdec_batch_status() looks)
  std::vector<hipEvent_t> ev;   // kEv events per timing slot; run k records into slot k % slots
  std::vector<hipEvent_t> chain_events;   // chain batches: one per motion step (the motion stream's progress, awaited by the pixel steps)
  std::vector<uint8_t> colour_timed;   // per slot: the colour stage of that run was recorded
  uint64_t runs = 0;
  hipStream_t last_stream = nullptr;
  bool ran = false;
  bool borrowed = false;        // owned by a hipdec_clips object (decoder_clips.inc): hipdec_batch_free leaves it alone, hipdec_batch_run is refused
  bool retired = false;         // its arena went to another batch (hipdec_batch_create_recycling): only status / timing / free remain
  uint32_t wave_share = 1;      // the CABAC work pool of this batch takes 1 / wave_share of the wave budget (launch sets of the decoder path overlap in pairs)
  ColorBatchState color;        // parameter blocks of hipdec_batch_to_rgb_all
  ColorBatchState color_scaled; // ... and of hipdec_batch_to_rgb_scaled_all (its own, so that a host alternating the two uploads nothing in the steady state)
  ColorBatchState color_tensor; // ... and of hipdec_batch_to_tensor
  ColorBatchState color_oriented; // ... and of the oriented forms (hipdec_batch_to_tensor_oriented, hipdec_batch_to_rgb_scaled_oriented_all)
  ColorBatchState color_margin;   // ... and the margin blocks of hipdec_batch_to_tensor_placed
  ColorBatchState color_packed;   // ... and of hipdec_batch_to_tensor_packed
  WarpState warp;                 // the table and the U8 intermediate of hipdec_batch_to_tensor_warped
  PhotoState photo;               // the tables, the U8 intermediate and the work memory of hipdec_batch_to_tensor_photo
  uint64_t max_pixels = 0;      // the limit given at creation (0: none): scaled outputs are held against it as well
  // decoder path (plugin): the output planes of every item staged in pinned host memory by ONE set of asynchronous copies behind the
  // kernels, so that N decoder instances sharing the batch do not queue N x 3 pageable device-to-host copies (stage_planes_to_host)
  struct HostItem { void* p = nullptr; size_t off[3] = {0, 0, 0}; const uint8_t* rgb = nullptr; };   // p points into one of host_chunks; rgb: tight RGB24 rows (resident RGB)
  std::vector<HostItem> host_items;
  // pinned chunks of ONE size (64 MiB; a larger item gets a chunk of its own), items sub-allocated at 256-B alignment: a launch set of 256
  // thumbnails pins one chunk instead of 256 x 16 MiB, and sets of any size recycle the same chunks from the pool
  std::vector<std::pair<void*, size_t>> host_chunks;
  // Resident RGB (drop-in through a libheif with the integration ops): when the host has been asking for interleaved RGB24 of
  // the images it decodes, the launch set runs the SAO kernel with the fused RGB24 emission (k_sao_rgb) into rgb_dev and stages the rows to pinned
  // host memory beside the planes: the colour conversion of libheif's pipeline then is a host copy instead of a kernel queued behind CABAC pools
  void* rgb_dev = nullptr;
  size_t rgb_capacity = 0;
  std::vector<size_t> rgb_off, rgb_stride;
  std::vector<std::pair<void*, size_t>> rgb_chunks;   // pinned
  std::atomic<int> rgb_consumed{0};
  bool fused_rgb = false;                 // the last hipdec_batch_run_rgb took the fused form (k_sao_rgb)
  // Pipelined chains (decoder_chains.inc): a chain launch set that is enqueued while earlier chains of the same tracks are still running.  Its CABAC
  // and residual launches need nothing of them and start at once; its motion derivation waits for their motion fields, its pixel steps for their
  // pictures.  The set keeps its streams until somebody has looked at its status (a stream handed back early would carry the NEXT set's CABAC
  // launch behind this set's pixel steps), and that look happens once, by whichever decoder instance needs a picture of the set first.
  std::vector<std::shared_ptr<hipdec_batch>> after;
  bool hold_streams = false;
  std::vector<hipStream_t> held_streams;
  bool motion_recorded = false;           // chain_events[0] stands behind the motion fields of ALL pictures
  std::mutex fin_mu;
  bool finished = false;
  int fin_rc = 0;
  std::string fin_err;
  // Waits for everything enqueued for THIS batch — not for the stream, which may already carry the next batch.
  hipError_t wait() const
  {
    hipError_t e = hipSuccess;
    if (uploaded) e = hipEventSynchronize(uploaded);
    if (e == hipSuccess && done_recorded) e = hipEventSynchronize(done);
    return e;
  }
  void mark_done(hipStream_t s)
  {
    if (done && hipEventRecord(done, s) == hipSuccess) done_recorded = true;
  }
  void release_staging()
  {
    if (!staging) return;
    if (uploaded) (void)hipEventSynchronize(uploaded);
    pinned_release(staging, staging_capacity);
    staging = nullptr;
    if (upload_dev) { arena_release(upload_dev, upload_dev_capacity); upload_dev = nullptr; }
  }
  ~hipdec_batch()
  {
    DeviceScope scope(device);
    if (arena || staging) (void)wait();   // nothing of this batch may still be running when the arena is recycled
    release_staging();
    for (hipStream_t hs : held_streams) stream_release(hs);
    for (auto& c : host_chunks) pinned_release(c.first, c.second);
    for (auto& c : rgb_chunks) pinned_release(c.first, c.second);
    if (rgb_dev) { arena_release(rgb_dev, rgb_capacity); rgb_note_unused((int)rgb_off.size() - rgb_consumed.load()); }
    color_batch_state_free(color);
    color_batch_state_free(color_scaled);
    color_batch_state_free(color_tensor);
    color_batch_state_free(color_oriented);
    color_batch_state_free(color_margin);
    color_batch_state_free(color_packed);
    warp_state_free(warp);
    photo_state_free(photo);
    if (arena) arena_release(arena, arena_capacity);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : chain_events) if (e) (void)hipEventDestroy(e);
    if (uploaded) (void)hipEventDestroy(uploaded);
    if (done) (void)hipEventDestroy(done);
    status_slot_release(host_status);
  }
};

namespace {

// The host side of "compressed bytes in host memory -> decode" (SURVEY.md §8d): header parsing (worker threads for large
// batches), staging and the upload.  Large upload regions go through pinned staging and ONE asynchronous copy on the
// library's upload stream, so that hipdec_batch_create() of batch k+1 overlaps the kernels of batch k; small ones (a still, the
// tiles of a grid photo) are copied synchronously from pageable memory, which is quicker than pinning.
// chains: the n items are consecutive samples of sequence tracks (BatchLayout::chain; items [first[t], first[t] + count[t]) belong to track t whose
// state is *seqs[t]): the batch may come out EMPTY (every sample was a RASL picture 8.3.3 drops) - then nothing is allocated
struct ChainPlan { int n_tracks; const int* first; const int* count; const SeqContext* const* seqs; int* bad_track; };
// after_plan: the caller's own rules over the parsed items (hipdec_album_create: the grid geometry of every photo), applied before anything is allocated
int build_batch(hipdec_batch& b, int n, const void* const* data, const size_t* sizes, uint64_t max_pixels, hipdec_batch* recycle = nullptr,
                const SeqContext* const* seqs = nullptr, const ChainPlan* chains = nullptr, const std::function<int(const hipdec_batch&)>* after_plan = nullptr)
{
  std::string err;
  b.device = active_device();
  b.max_pixels = max_pixels;
  int rc = chains ? layout_batch_plan_chains(b, chains->n_tracks, chains->first, chains->count, data, sizes, max_pixels, err, chains->seqs, chains->bad_track)
                  : layout_batch_plan(b, n, data, sizes, max_pixels, err, seqs);
  if (rc != HIPDEC_OK) return set_error(rc, "%s", err.c_str());
  if (after_plan) if (int vrc = (*after_plan)(b)) return vrc;
  if (b.pics.empty()) return 0;
  HIPDEC_CHECK_HIP(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
  b.host_status = status_slot_acquire();
  if (!b.host_status) return set_error(HIPDEC_ERR_MEMORY, "batch_create: more than 4096 live batches (no pinned status slot left)");
  *b.host_status = 0;
  // a retired batch of the same shape hands its arena over (hipdec_batch_create_recycling): the upload is ordered behind
  // everything that batch still has in flight, so one arena serves a stream of batches
  hipEvent_t after = nullptr;
  if (recycle && recycle->arena && recycle->arena_capacity >= b.arena_size && recycle->device == b.device) {
    b.arena = recycle->arena; b.arena_capacity = recycle->arena_capacity;
    recycle->arena = nullptr; recycle->arena_capacity = 0;
    if (recycle->done_recorded) after = recycle->done;
    recycle->retired = true;
  }
  // if anything below fails, the arena goes back to the pool with this batch: not before the retired batch's kernels have left it
  struct TakeoverGuard {
    hipEvent_t after; bool ok;
    ~TakeoverGuard() { if (!ok && after) (void)hipEventSynchronize(after); }
  } takeover{after, false};
  static const bool sync_upload = getenv("HIPDEC_SYNC_UPLOAD") != nullptr;   // profiling knob: one stream, no cross-stream event waits
  // (a chain that is enqueued beside chains in flight never takes the synchronous copy: hipMemcpy from pageable memory waits for the device - measured,
  //  80 ms per chain of 16 720p pictures, i.e. for everything in flight)
  if ((b.upload_size > (size_t(4) << 20) || b.hold_streams) && !sync_upload) {
    HIPDEC_CHECK_HIP(pinned_acquire(&b.staging, b.upload_size, &b.staging_capacity));
    if (!b.arena) HIPDEC_CHECK_HIP(arena_acquire((void**)&b.arena, b.arena_size, &b.arena_capacity));   // (first: a chain's reference tables hold addresses inside it)
    layout_batch_fill(b, data, sizes, (uint8_t*)b.staging, (uint64_t)(uintptr_t)b.arena);
    HIPDEC_CHECK_HIP(hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming));
    hipStream_t us = upload_stream();
    // An arena taken over from a batch whose kernels are still running cannot receive the upload yet: the bytes cross PCIe NOW into a bounce
    // buffer in HBM (beside those kernels) and move into the arena with a device copy once the predecessor has finished - 2 GB per 2048 4K
    // stills are ~ 40 ms of link time against ~ 1 ms of HBM copy between two batches.  No memory for the bounce buffer: the upload waits.
    static const bool no_bounce = getenv("HIPDEC_NO_UPLOAD_BOUNCE") != nullptr;   // A/B knob
    if (after && !no_bounce && arena_acquire(&b.upload_dev, b.upload_size, &b.upload_dev_capacity) != hipSuccess) { b.upload_dev = nullptr; (void)hipGetLastError(); }
    if (after && b.upload_dev) {
      HIPDEC_CHECK_HIP(hipMemcpyAsync(b.upload_dev, b.staging, b.upload_size, hipMemcpyHostToDevice, us));
      HIPDEC_CHECK_HIP(hipStreamWaitEvent(us, after, 0));
      HIPDEC_CHECK_HIP(hipMemcpyAsync(b.arena, b.upload_dev, b.upload_size, hipMemcpyDeviceToDevice, us));
    } else {
      if (after) HIPDEC_CHECK_HIP(hipStreamWaitEvent(us, after, 0));
      HIPDEC_CHECK_HIP(hipMemcpyAsync(b.arena, b.staging, b.upload_size, hipMemcpyHostToDevice, us));
    }
    HIPDEC_CHECK_HIP(hipEventRecord(b.uploaded, us));
  } else {
    std::vector<uint8_t> host(b.upload_size);
    if (!b.arena) HIPDEC_CHECK_HIP(arena_acquire((void**)&b.arena, b.arena_size, &b.arena_capacity));
    layout_batch_fill(b, data, sizes, host.data(), (uint64_t)(uintptr_t)b.arena);
    if (after) HIPDEC_CHECK_HIP(hipEventSynchronize(after));
    HIPDEC_CHECK_HIP(hipMemcpy(b.arena, host.data(), b.upload_size, hipMemcpyHostToDevice));
  }
  b.ev.assign(kEv, nullptr);
  b.colour_timed.assign(1, 0);
  for (auto& e : b.ev) HIPDEC_CHECK_HIP(hipEventCreate(&e));
  takeover.ok = true;
  return 0;
}

// The stream follow-up work of a batch (colour stage, packs, pastes) goes on: the caller's, made to wait for the batch's last recorded
// work when that was enqueued elsewhere — with hipdec_set_stage_overlap(1) the pixel stages of a run leave the caller's stream for the
// post stream, so a copy queued on the caller's stream right behind hipdec_batch_run() would otherwise read unfinished planes
//  — or the batch's own last stream.
hipStream_t follow_stream(hipdec_batch* b, void* stream)
{
  if (!stream) return b->last_stream ? b->last_stream : default_stream();
  hipStream_t s = (hipStream_t)stream;
  if (s != b->last_stream && b->done_recorded) (void)hipStreamWaitEvent(s, b->done, 0);
  return s;
}

}  // namespace
namespace hipdec { hipStream_t batch_follow_stream(hipdec_batch* b, hipStream_t s) { return follow_stream(b, (void*)s); } }
namespace {

int launch_all(hipdec_batch& b, hipStream_t s, const void* fused_rgb_params = nullptr)
{
  const int n = (int)b.params.size();
  ParseArgs pa{};
  pa.pics = (const PicParams*)(b.arena + b.off_pics); pa.subs = (const Substream*)(b.arena + b.off_subs);
  pa.waves = (const ParseWave*)(b.arena + b.off_waves); pa.num_waves = b.num_waves; pa.arena = b.arena;
  pa.progress = (uint32_t*)(b.arena + b.off_progress); pa.ctx_store = b.arena + b.off_ctx;
  pa.ticket = (uint32_t*)(b.arena + b.off_ticket); pa.status = (int32_t*)(b.arena + b.off_status);
  if (b.pool) {
    // pool size: every pool wave must be resident, so the batches in flight share the wave slots (runtime.hip); measured on
    // MI355X, 1024 4K stills: 7168 waves for one batch, 2 x 3584 for two overlapping ones (2 x 4096 oversubscribes and
    // loses 20 %)
    uint32_t waves = getenv("HIPDEC_POOL_WAVES") ? (uint32_t)atoi(getenv("HIPDEC_POOL_WAVES")) : parse_wave_budget() / (b.wave_share ? b.wave_share : 1u);
    waves = waves > b.num_subs ? b.num_subs : waves;
    pa.num_waves = waves < 1 ? 1 : waves;
  }
  // a row hands its wave back after every CTB: the ready queue then advances all rows breadth-first and rows rarely run into
  // the row above (measured: parse 698 -> 591 ms against "run until blocked")
  pa.yield_ctbs = getenv("HIPDEC_POOL_YIELD") ? (uint32_t)atoi(getenv("HIPDEC_POOL_YIELD")) : 1;
  pa.wake_hyst = getenv("HIPDEC_POOL_HYST") ? (uint32_t)atoi(getenv("HIPDEC_POOL_HYST")) : 0u;
  pa.general_chroma = 0;
  for (const PicParams& P : b.params) if (P.chroma_format_idc >= 2) pa.general_chroma = 1;
  pa.inter = b.any_inter ? 1 : 0;
  pa.pool = b.pool; pa.queue_cap = b.queue_cap; pa.num_subs = b.num_subs;
  pa.waitneed = (uint32_t*)(b.arena + b.off_waitneed); pa.resume_k = (uint32_t*)(b.arena + b.off_resume_k);
  pa.queue = (uint32_t*)(b.arena + b.off_queue); pa.qctl = (uint32_t*)(b.arena + b.off_qctl); pa.saved = (uint32_t*)(b.arena + b.off_saved);
  ReconArgs ra{(const PicParams*)(b.arena + b.off_pics), (const ReconWave*)(b.arena + b.off_rwaves), b.num_rwaves, b.arena,
               (uint32_t*)(b.arena + b.off_row_progress), (uint32_t*)(b.arena + b.off_ticket) + 1, (int32_t*)(b.arena + b.off_status)};
  FilterArgs fa{(const PicParams*)(b.arena + b.off_pics), b.arena, (const int32_t*)(b.arena + b.off_status)};
  const bool dbg = getenv("HIPDEC_DEBUG_SYNC") != nullptr;  // isolate a faulting kernel
  auto step = [&](const char* what) -> int {
    if (!dbg) return 0;
    fprintf(stderr, "[hipdec] %s ...\n", what); fflush(stderr);
    hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[hipdec] %s: %s\n", what, hipGetErrorString(e)); fflush(stderr);
    return e == hipSuccess ? 0 : set_error(HIPDEC_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  };
  const size_t slot = b.runs % (b.ev.size() / kEv);
  hipEvent_t* ev = b.ev.data() + kEv * slot;
  b.colour_timed[slot] = 0;
  b.runs++;
  if (b.uploaded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(s, b.uploaded, 0));
  // Two-stage pipeline across batches (hipdec_set_stage_overlap): the CABAC kernel runs on the caller's stream, everything behind it on the
  // device's post stream.  With two batches alternating, batch k+1's parse — scalar / vector issue bound, its dependency tail leaves the
  // chip half empty — overlaps batch k's reconstruction, filters and colour stage (VALU + HBM).  A batch's own previous run must have
  // left the arena before the control words are zeroed again.
  const bool split = stage_overlap();
  hipStream_t ps = split ? post_stream() : s;
  if (split && b.done_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(s, b.done, 0));
  HIPDEC_CHECK_HIP(hipMemsetAsync(b.arena + b.off_ctrl, 0, b.ctrl_size, s));
  HIPDEC_CHECK_HIP(hipEventRecord(ev[0], s));
  if (int rc = step("memset")) return rc;
#ifdef HIPDEC_POOL_TRACE   // measurement build: per pool wave {start, end of its last row, last look at the queue, time waiting for work, rows run, time in rows}
  {                        // in 100 MHz ticks; the previous run's table is appended to $HIPDEC_POOL_TRACE (binary, 32 x uint64 per wave - [8 + k]: time waiting for work in the k-th 42 ms of its life -, 8192 waves per run)
    static unsigned long long* trace = nullptr;
    const size_t bytes = 8192 * 32 * sizeof(unsigned long long);
    if (!trace) { HIPDEC_CHECK_HIP(hipMalloc((void**)&trace, bytes)); HIPDEC_CHECK_HIP(hipMemset(trace, 0, bytes)); }
    else if (const char* path = getenv("HIPDEC_POOL_TRACE")) {
      HIPDEC_CHECK_HIP(hipDeviceSynchronize());
      std::vector<unsigned long long> h(8192 * 32);
      HIPDEC_CHECK_HIP(hipMemcpy(h.data(), trace, bytes, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(path, "ab")) { fwrite(h.data(), 1, bytes, f); fclose(f); }
      HIPDEC_CHECK_HIP(hipMemset(trace, 0, bytes));
    }
    pa.trace = trace;
  }
#endif
  launch_parse(pa, s);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[1], s));
  if (int rc = step("parse")) return rc;
  if (split) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, ev[1], 0));
  static const bool parse_only = getenv("HIPDEC_DEBUG_PARSE_ONLY") != nullptr;   // tuning knob: isolate the CABAC kernel
  if (!parse_only) launch_residual(fa, n, b.max_ctbs, pa.general_chroma != 0, ps);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[2], ps));
  if (int rc = step("residual")) return rc;
  if (!parse_only && b.chain) {
    // A chain (consecutive samples of one track, parsed and inverse-transformed together above).  Motion derivation needs the parser's output and
    // the collocated picture's motion field only, so the motion steps run on a stream of their own behind the parser, beside the pixel steps of
    // earlier pictures; a pixel step (prediction, reconstruction, filters of pictures that do not predict from each other) waits for the motion
    // fields of its pictures, and stream order makes every reference picture - earlier items of this batch among them - complete.
    static const bool motion_by_steps = getenv("HIPDEC_CHAIN_MOTION_STEPS") != nullptr;   // A/B knob: one k_motion launch per motion step (the form before the
                                                                                          // kernel waited for its collocated picture's rows itself)
    if (b.any_inter && !motion_by_steps) {
      // the motion fields of ALL pictures with one launch on a stream of its own (kernels.h: launch_chain_motion_all), the pixel steps behind it
      hipStream_t ms = stream_acquire();
      if (b.chain_events.empty()) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { stream_release(ms); return set_error(HIPDEC_ERR_DEVICE, "chain: no event"); }
        b.chain_events.push_back(e);
      }
      HIPDEC_CHECK_HIP(hipStreamWaitEvent(ms, ev[1], 0));
      for (const auto& pred : b.after) {   // collocated pictures of chains still in flight: their motion fields
        if (pred->motion_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ms, pred->chain_events[0], 0));
        else if (pred->done_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ms, pred->done, 0));
      }
      launch_chain_motion_all(b, b.arena, ms);
      HIPDEC_CHECK_HIP(hipEventRecord(b.chain_events[0], ms));
      b.motion_recorded = true;
      if (b.hold_streams) b.held_streams.push_back(ms); else stream_release(ms);
      for (const auto& pred : b.after)     // reference pictures of chains still in flight
        if (pred->done_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, pred->done, 0));
      bool waited = false;
      for (size_t k = 0; k < b.pixel_steps.size(); k++) {
        if (b.pixel_steps[k].any_inter && !waited) { HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, b.chain_events[0], 0)); waited = true; }
        launch_chain_pixels(b, b.arena, (int)k, ps);
      }
      if (!waited) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, b.chain_events[0], 0));   // nothing of this batch outlives its `done` event
      HIPDEC_CHECK_HIP(hipEventRecord(ev[3], ps));
      HIPDEC_CHECK_HIP(hipEventRecord(ev[4], ps));
      HIPDEC_CHECK_HIP(hipEventRecord(ev[5], ps));
      if (int rc = step("chain pixel stages")) return rc;
      HIPDEC_CHECK_HIP(hipGetLastError());
      // (a set left in flight queues NO copy behind its kernels: a DMA copy that waits for the pixel steps holds its copy engine's queue, and the upload
      //  of the next set - whose CABAC launch is to run beside those pixel steps - sits behind it; batch_finish copies once the kernels are done)
      if (!b.hold_streams) HIPDEC_CHECK_HIP(hipMemcpyAsync(b.host_status, b.arena + b.off_status, sizeof(int32_t), hipMemcpyDeviceToHost, ps));
      b.last_stream = ps;
      b.mark_done(ps);
      return 0;
    }
    for (const auto& pred : b.after)       // (the forms below keep the simple order: everything of this chain's later stages behind the chains in flight)
      if (pred->done_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, pred->done, 0));
    hipStream_t ms = nullptr;
    if (b.any_inter && b.motion_steps.size() > 1) {
      ms = stream_acquire();
      while (b.chain_events.size() < b.motion_steps.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { stream_release(ms); return set_error(HIPDEC_ERR_DEVICE, "chain: no event"); }
        b.chain_events.push_back(e);
      }
      HIPDEC_CHECK_HIP(hipStreamWaitEvent(ms, ev[1], 0));
      for (const auto& pred : b.after) if (pred->done_recorded) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ms, pred->done, 0));
      for (size_t k = 0; k < b.motion_steps.size(); k++) {
        launch_chain_motion(b, b.arena, (int)k, ms);
        HIPDEC_CHECK_HIP(hipEventRecord(b.chain_events[k], ms));
      }
      stream_release(ms);   // (everything it carries is ordered into `ps` through the events below)
    }
    int motion_done = 0;
    for (size_t k = 0; k < b.pixel_steps.size(); k++) {
      const BatchLayout::ChainStep& st = b.pixel_steps[k];
      const int need = st.motion_need;
      if (ms) { if (st.any_inter) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, b.chain_events[(size_t)need - 1], 0)); }
      else for (; motion_done < need; motion_done++) launch_chain_motion(b, b.arena, motion_done, ps);
      launch_chain_pixels(b, b.arena, (int)k, ps);
    }
    if (ms) HIPDEC_CHECK_HIP(hipStreamWaitEvent(ps, b.chain_events[b.motion_steps.size() - 1], 0));   // nothing of this batch outlives its `done` event
    HIPDEC_CHECK_HIP(hipEventRecord(ev[3], ps));
    HIPDEC_CHECK_HIP(hipEventRecord(ev[4], ps));
    HIPDEC_CHECK_HIP(hipEventRecord(ev[5], ps));
    if (int rc = step("chain pixel stages")) return rc;
    HIPDEC_CHECK_HIP(hipGetLastError());
    if (!b.hold_streams) HIPDEC_CHECK_HIP(hipMemcpyAsync(b.host_status, b.arena + b.off_status, sizeof(int32_t), hipMemcpyDeviceToHost, ps));
    b.last_stream = ps;
    b.mark_done(ps);
    return 0;
  }
  if (!parse_only && b.any_inter) {
    // P pictures: motion vectors (merge / AMVP candidates: a 2-CTB wavefront over CTB rows), then the motion-compensated prediction of every
    // inter coded sample into the reconstruction planes; k_recon adds the residuals and predicts the intra blocks around them
    MotionArgs ma{(const PicParams*)(b.arena + b.off_pics), (const RowDesc*)(b.arena + b.off_rows), b.num_rows, b.arena,
                  (uint32_t*)(b.arena + b.off_row_progress), (uint32_t*)(b.arena + b.off_ticket) + 2, (int32_t*)(b.arena + b.off_status)};
    launch_motion(ma, ps);
    launch_mc(fa, n, b.max_w, b.max_h, b.wide, ps, inter_residual_in_mc());
    ra.inter_from_plane = inter_residual_in_mc() ? 1u : 0u;
    if (int rc = step("motion + mc")) return rc;
  }
  if (!parse_only) launch_recon(ra, b.wide, ps, b.any_inter, b.general_chroma ? 1 : 0);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[3], ps));
  if (int rc = step("recon")) return rc;
  if (!parse_only) launch_deblock(fa, n, b.max_w, b.max_h, b.wide, ps, !b.any_inter && !pa.general_chroma);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[4], ps));
  if (int rc = step("deblock")) return rc;
  if (!parse_only) {
    bool may_keep = false, restricted = false;
    for (const PicParams& P : b.params) {
      if (P.transquant_bypass_enabled || (P.pcm_enabled && P.pcm_loop_filter_disabled)) may_keep = true;
      if (!P.sao_free_neighbours) restricted = true;
    }
    if (fused_rgb_params)   // SAO + crop + RGB24 in one pass
      launch_sao_rgb(fa, fused_rgb_params, n, b.max_ow, b.max_oh, ps, may_keep, restricted, b.params.data(),
                     b.color.host.size() == (size_t)n * sizeof(colordev::ColorParams) ? b.color.host.data() : nullptr);
    else launch_sao(fa, n, b.max_ow, b.max_oh, b.wide, ps, may_keep, restricted);
  }
  HIPDEC_CHECK_HIP(hipEventRecord(ev[5], ps));
  if (int rc = step("sao")) return rc;
  HIPDEC_CHECK_HIP(hipGetLastError());
  HIPDEC_CHECK_HIP(hipMemcpyAsync(b.host_status, b.arena + b.off_status, sizeof(int32_t), hipMemcpyDeviceToHost, ps));
  b.last_stream = ps;     // the colour stage, packs and plane reads of this run follow its last kernel
  b.mark_done(ps);
  return 0;
}

const char* dev_err_name(int code)
{
  switch (code & 0xff) {
    case DEV_ERR_TERMINATE: return "CABAC substream did not terminate where the slice header says (desynchronised bitstream)";
    case DEV_ERR_BITSTREAM_END: return "CABAC read past the end of a substream";
    case DEV_ERR_SYNTAX: return "syntax element out of range";
    case DEV_ERR_TIMEOUT: return "dependency wait timed out / aborted";
    default: return "unknown device error";
  }
}

// The decoder path's hand-over: every item's cropped planes, tight rows, into a pinned buffer of its own (pooled), queued on the
// launch set's stream behind its kernels.  hipdec_decoder_read_plane() then is a host memcpy into libheif's plane — in parallel on the
// application's threads — instead of one synchronous pageable device-to-host copy per plane and instance.
int stage_planes_to_host(hipdec_batch& b, hipStream_t s)
{
  static const bool off = getenv("HIPDEC_NO_HOST_STAGING") != nullptr;
  if (off) return 0;
  const size_t es = b.wide ? 2 : 1;
  constexpr size_t kChunk = size_t(64) << 20;
  std::vector<hipdec_batch::HostItem> items(b.params.size());
  std::vector<size_t> need;                       // bytes used of chunk k
  std::vector<std::pair<int, size_t>> place(b.params.size(), {-1, 0});   // item -> (chunk, offset)
  for (size_t i = 0; i < b.params.size(); i++) {
    const PicParams& P = b.params[i];
    size_t total = 0;
    for (int c = 0; c < (P.chroma_format_idc ? 3 : 1); c++) {
      items[i].off[c] = total;
      total += (size_t)(c ? P.out_cwidth : P.out_width) * es * (size_t)(c ? P.out_cheight : P.out_height);
      total = (total + 255) & ~size_t(255);
    }
    if (!total) continue;
    if (need.empty() || need.back() + total > std::max(kChunk, need.back() ? kChunk : total)) need.push_back(0);
    place[i] = {(int)need.size() - 1, need.back()};
    need.back() += total;
  }
  if (need.empty()) return 0;
  // chunks this batch already holds are reused (a second run over the same arena); missing ones come from the pool
  bool ok = true;
  for (size_t k = 0; k < need.size() && ok; k++) {
    const size_t want = std::max(kChunk, need[k]);
    if (k < b.host_chunks.size() && b.host_chunks[k].second >= want) continue;
    if (k < b.host_chunks.size()) { pinned_release(b.host_chunks[k].first, b.host_chunks[k].second); b.host_chunks[k] = {nullptr, 0}; }
    else b.host_chunks.emplace_back(nullptr, 0);
    if (pinned_acquire(&b.host_chunks[k].first, want, &b.host_chunks[k].second) != hipSuccess) { (void)hipGetLastError(); b.host_chunks[k] = {nullptr, 0}; ok = false; }
  }
  if (!ok) {
    // no pinned memory even after the pool was emptied (pinned_acquire retries once): the instances read their planes straight from the
    // device instead (hipdec_batch_read_plane's unstaged path) - slower, but not an error
    for (auto& c : b.host_chunks) pinned_release(c.first, c.second);
    b.host_chunks.clear();
    b.host_items.clear();
    return 0;
  }
  for (size_t i = 0; i < b.params.size(); i++) {
    if (place[i].first < 0) continue;
    const PicParams& P = b.params[i];
    hipdec_batch::HostItem& h = items[i];
    h.p = (uint8_t*)b.host_chunks[(size_t)place[i].first].first + place[i].second;
    for (int c = 0; c < (P.chroma_format_idc ? 3 : 1); c++) {
      const size_t w = (size_t)(c ? P.out_cwidth : P.out_width) * es, hh = (size_t)(c ? P.out_cheight : P.out_height);
      if (!w || !hh) continue;
      if (P.out_stride[c] == w) HIPDEC_CHECK_HIP(hipMemcpyAsync((uint8_t*)h.p + h.off[c], b.arena + P.off_out[c], w * hh, hipMemcpyDeviceToHost, s));   // (the usual case: one DMA)
      else HIPDEC_CHECK_HIP(hipMemcpy2DAsync((uint8_t*)h.p + h.off[c], w, b.arena + P.off_out[c], P.out_stride[c], w, hh, hipMemcpyDeviceToHost, s));
    }
  }
  // resident RGB: the fused colour stage's rows, tight, one pinned chunk set of their own
  if (b.rgb_dev && b.rgb_off.size() == b.params.size()) {
    std::vector<size_t> rneed;
    std::vector<std::pair<int, size_t>> rplace(b.params.size(), {-1, 0});
    for (size_t i = 0; i < b.params.size(); i++) {
      const size_t total = ((size_t)b.params[i].out_width * 3 * (size_t)b.params[i].out_height + 255) & ~size_t(255);
      if (!total) continue;
      if (rneed.empty() || rneed.back() + total > std::max(kChunk, rneed.back() ? kChunk : total)) rneed.push_back(0);
      rplace[i] = {(int)rneed.size() - 1, rneed.back()};
      rneed.back() += total;
    }
    bool rok = true;
    for (size_t k = 0; k < rneed.size() && rok; k++) {
      const size_t want = std::max(kChunk, rneed[k]);
      if (k < b.rgb_chunks.size() && b.rgb_chunks[k].second >= want) continue;
      if (k < b.rgb_chunks.size()) { pinned_release(b.rgb_chunks[k].first, b.rgb_chunks[k].second); b.rgb_chunks[k] = {nullptr, 0}; }
      else b.rgb_chunks.emplace_back(nullptr, 0);
      if (pinned_acquire(&b.rgb_chunks[k].first, want, &b.rgb_chunks[k].second) != hipSuccess) { (void)hipGetLastError(); b.rgb_chunks[k] = {nullptr, 0}; rok = false; }
    }
    if (rok)
      for (size_t i = 0; i < b.params.size(); i++) {
        if (rplace[i].first < 0) continue;
        const PicParams& P = b.params[i];
        uint8_t* dst = (uint8_t*)b.rgb_chunks[(size_t)rplace[i].first].first + rplace[i].second;
        const size_t row = (size_t)P.out_width * 3;
        if (b.rgb_stride[i] == row) HIPDEC_CHECK_HIP(hipMemcpyAsync(dst, (uint8_t*)b.rgb_dev + b.rgb_off[i], row * (size_t)P.out_height, hipMemcpyDeviceToHost, s));
        else HIPDEC_CHECK_HIP(hipMemcpy2DAsync(dst, row, (uint8_t*)b.rgb_dev + b.rgb_off[i], b.rgb_stride[i], row, (size_t)P.out_height, hipMemcpyDeviceToHost, s));
        items[i].rgb = dst;
      }
    else { for (auto& c : b.rgb_chunks) pinned_release(c.first, c.second); b.rgb_chunks.clear(); }
  }
  b.host_items.swap(items);
  b.mark_done(s);
  return 0;
}

int copy_plane_d2h(const hipdec_batch& b, size_t off, uint32_t stride, int w, int h, void* dst, size_t dst_stride)
{
  const size_t es = b.wide ? 2 : 1;
  if (w <= 0 || h <= 0) return 0;
  // (a stride below the row length would put the last row past the end of a buffer of h * stride bytes)
  if (dst_stride < (size_t)w * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane: dst_stride %zu is smaller than a row of %zu bytes", dst_stride, (size_t)w * es);
  HIPDEC_CHECK_HIP(hipMemcpy2D(dst, dst_stride, b.arena + off, stride, (size_t)w * es, (size_t)h, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int hipdec_batch_create(hipdec_batch** out, int n, const void* const* data, const size_t* sizes, uint64_t max_image_size_pixels)
{
  if (!out || n <= 0 || !data || !sizes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_create: bad arguments");
  *out = nullptr;
  if (int rc = ensure_init()) return rc;
  return guarded("batch_create", [&]() -> int {
    std::unique_ptr<hipdec_batch> b(new hipdec_batch());
    if (int rc = build_batch(*b, n, data, sizes, max_image_size_pixels)) return rc;
    *out = b.release();
    return 0;
  });
}

int hipdec_batch_create_recycling(hipdec_batch** out, int n, const void* const* data, const size_t* sizes, uint64_t max_image_size_pixels,
                                  hipdec_batch* recycle)
{
  if (!out || n <= 0 || !data || !sizes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_create: bad arguments");
  *out = nullptr;
  if (int rc = ensure_init()) return rc;
  return guarded("batch_create", [&]() -> int {
    std::unique_ptr<hipdec_batch> b(new hipdec_batch());
    if (int rc = build_batch(*b, n, data, sizes, max_image_size_pixels, recycle)) return rc;
    *out = b.release();
    return 0;
  });
}

void hipdec_batch_free(hipdec_batch* b) { if (b && b->borrowed) return; delete b; }
int hipdec_batch_count(const hipdec_batch* b) { return b ? (int)b->pics.size() : 0; }

int hipdec_batch_info(const hipdec_batch* b, int i, hipdec_image_info* info)
{
  if (!b || !info || i < 0 || i >= (int)b->pics.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_info: bad arguments");
  *info = b->pics[i].info;
  return 0;
}

int hipdec_batch_run(hipdec_batch* b, void* stream)
{
  if (!b) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_run: NULL batch");
  if (b->borrowed) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_run: the batch is borrowed from a hipdec_clips object (hipdec_clips_run runs it)");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_run: the batch's arena was handed to another batch");
  if (int rc = ensure_init()) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  b->last_stream = s;
  b->ran = true;
  return launch_all(*b, s);   // (may move last_stream to the post stream)
}

int hipdec_batch_status(hipdec_batch* b)
{
  if (!b || !b->ran) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "batch_status: batch has not been run");
  DeviceScope scope(b->device);
  if (int rc = ensure_init()) return rc;
  hipError_t e = b->wait();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "decode kernels failed: %s", hipGetErrorString(e));
  b->release_staging();
  const int32_t st = *b->host_status;
  if (st != 0) return set_error(HIPDEC_ERR_DECODE, "device decode error 0x%x: %s", st, dev_err_name(st));
  return 0;
}

int hipdec_batch_read_plane(hipdec_batch* b, int i, int c, void* dst, size_t dst_stride)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || c < 0 || c > 2 || !dst) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane: the batch's arena was handed to another batch");
  const PicParams& P = b->params[i];
  if (c > 0 && !P.chroma_format_idc) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane: monochrome image has no chroma planes");
  return copy_plane_d2h(*b, P.off_out[c], P.out_stride[c], c ? P.out_cwidth : P.out_width, c ? P.out_cheight : P.out_height, dst, dst_stride);
}

int hipdec_batch_device_plane(hipdec_batch* b, int i, int c, const void** dptr, size_t* stride)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || c < 0 || c > 2 || !dptr || !stride) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "device_plane: bad arguments");
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "device_plane: the batch's arena was handed to another batch");
  const PicParams& P = b->params[i];
  *dptr = b->arena + P.off_out[c];
  *stride = P.out_stride[c];
  return 0;
}

size_t hipdec_batch_item_packed_bytes(const hipdec_batch* b, int i)
{
  if (!b || i < 0 || i >= (int)b->pics.size()) return 0;
  const PicParams& P = b->params[i];
  const size_t es = b->wide ? 2 : 1;
  return ((size_t)P.out_width * P.out_height + 2 * (size_t)P.out_cwidth * P.out_cheight) * es;
}

int hipdec_batch_pack_item(hipdec_batch* b, int i, void* dst_dev, size_t dst_bytes, void* stream)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || !dst_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "pack_item: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "pack_item: the batch's arena was handed to another batch");
  if (dst_bytes < hipdec_batch_item_packed_bytes(b, i)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "pack_item: destination too small");
  const PicParams& P = b->params[i];
  const size_t es = b->wide ? 2 : 1;
  hipStream_t s = follow_stream(b, stream);
  uint8_t* dst = (uint8_t*)dst_dev;
  for (int c = 0; c < (P.chroma_format_idc ? 3 : 1); c++) {
    const size_t w = c ? P.out_cwidth : P.out_width, h = c ? P.out_cheight : P.out_height;
    if (w && h) HIPDEC_CHECK_HIP(hipMemcpy2DAsync(dst, w * es, b->arena + P.off_out[c], P.out_stride[c], w * es, h, hipMemcpyDeviceToDevice, s));
    dst += w * h * es;
  }
  b->mark_done(s);
  return 0;
}

int hipdec_copy2d_d2d(void* dst_dev, size_t dst_stride, const void* src_dev, size_t src_stride, size_t width_bytes, size_t height, void* stream)
{
  if (!dst_dev || !src_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "copy2d: NULL pointer");
  if (int rc = ensure_init()) return rc;
  if (!width_bytes || !height) return 0;
  HIPDEC_CHECK_HIP(hipMemcpy2DAsync(dst_dev, dst_stride, src_dev, src_stride, width_bytes, height, hipMemcpyDeviceToDevice,
                                    stream ? (hipStream_t)stream : default_stream()));
  return 0;
}

}  // extern "C"

namespace {

// hipdec_batch_to_rgb, and - with a scale request - hipdec_batch_to_rgb_scaled: the same argument checks and planner rules; the request makes the colour
// entry points end in the fused scale + colour kernel (color.hip).  Box presents the planes as the 4:4:4 image they are scaled to.
struct ScaleRequest { int ow, oh, filter; };
// the Pillow-exact filters (include/heif_hipdec.h): taken by the tensor forms and the RGB24 forms, through k_resample (color.hip)
inline bool resample_filter(int filter) { return filter == HIPDEC_SCALE_BILINEAR || filter == HIPDEC_SCALE_BICUBIC; }
int copy_rows_to_host(void* dst, size_t dst_stride, const void* dsrc, size_t src_stride, size_t row_bytes, int rows, hipStream_t s);   // decoder_color_boundary.inc
// The planes one picture hands to the colour entry points: a decoded item of a batch (hipdec_batch_to_rgb*), or the composed canvas of a photo of an
// album (hipdec_album_to_rgb*, decoder_album.inc).  info: the VUI colour description and the bit depth.
struct RgbSource {
  const uint8_t* plane[3]; size_t stride[3];
  int width, height, chroma_format_idc;
  bool wide;
  const hipdec_image_info* info;
  uint64_t max_pixels;
};
// resolve_stream(): called once, when the argument checks have passed, for the stream the launch goes on
template <class ResolveStream>
int source_to_rgb(const RgbSource& S, int out_chroma, void* out_dev, size_t out_stride, const ScaleRequest* rq, ResolveStream&& resolve_stream)
{
  int cf = S.chroma_format_idc;   // the chroma format the planner rules below see
  const hipdec_image_info& I = *S.info;
  struct ScaleScope { bool on; ~ScaleScope() { if (on) color_scale_clear(); } } scale_scope{rq != nullptr};
  // a request serves exactly ONE launch and the entry point that takes it clears it: one that did not (it launched a full-size kernel) is an error here
  auto taken = [&](int rc) -> int {
    if (!rc && rq && color_scale_pending()) return set_error(HIPDEC_ERR_UNSUPPORTED, "to_rgb_scaled: the colour entry point did not take the scale request");
    return rc;
  };
  if (rq) {
    if (rq->ow < 1 || rq->oh < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb_scaled: output size %d x %d", rq->ow, rq->oh);
    if (rq->filter != HIPDEC_SCALE_NEAREST && rq->filter != HIPDEC_SCALE_BOX) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb_scaled: unknown filter %d", rq->filter);
    if (S.max_pixels && (uint64_t)rq->ow * (uint64_t)rq->oh > S.max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "to_rgb_scaled: output of %d x %d pixels exceeds max_image_size_pixels", rq->ow, rq->oh);
    color_scale_request(rq->ow, rq->oh, rq->filter, S.chroma_format_idc == 1 || S.chroma_format_idc == 2 ? 1 : 0, S.chroma_format_idc == 1 ? 1 : 0);
    if (rq->filter == HIPDEC_SCALE_BOX && cf) cf = 3;   // (box: the 4:4:4 image the planes are scaled to)
  }
  {
    const size_t bpp = out_chroma == 10 ? 3 : (out_chroma == 11 ? 4 : (out_chroma == 12 || out_chroma == 14 ? 6 : 0));
    const size_t row_px = rq ? (size_t)rq->ow : (size_t)S.width;
    if (bpp && out_stride < row_px * bpp)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb: out_stride %zu is smaller than a row of %zu bytes", out_stride, row_px * bpp);
  }
  if (!cf) {   // Op_mono_to_RGB24_32: 8-bit only, as in the reference
    if (S.wide || (out_chroma != 10 && out_chroma != 11)) return set_error(HIPDEC_ERR_UNSUPPORTED, "to_rgb: monochrome input goes to 8-bit RGB / RGBA only");
    void* ms = resolve_stream();
    return taken(hipdec_color_mono_to_rgb24(S.plane[0], S.stride[0], nullptr, 0, S.width, S.height, out_dev, out_stride, out_chroma == 11, ms));
  }
  // the decoder reports the VUI colour description exactly as the libde265 plugin would attach it
  hipdec_nclx nclx{1, I.colour_primaries, I.transfer_characteristics, I.matrix_coeffs, I.full_range_flag};
  const uint8_t* y = S.plane[0]; const uint8_t* cb = S.plane[1]; const uint8_t* cr = S.plane[2];
  void* s = resolve_stream();
  if ((out_chroma == 10 || out_chroma == 11) && S.wide) {
    // > 8-bit planes to 8-bit RGB(A): one of the two chains of the planner (nearest-neighbour upsampling is this entry point's), fused into one pass
    const int m = I.matrix_coeffs == 2 ? 6 : I.matrix_coeffs;
    const int sdr_first = cf == 1 && I.full_range_flag && m != 0 && m != 8;
    return taken(hipdec_color_hdr_to_rgb24(y, S.stride[0], cb, S.stride[1], cr, S.stride[2], S.width, S.height, I.bit_depth_luma,
                                     cf, &nclx, out_dev, out_stride, out_chroma == 11, sdr_first, s));
  }
  if (out_chroma == 10 || out_chroma == 11) {
    // planner rule: integer op only for full range and a matrix it accepts
    const int m = I.matrix_coeffs == 2 ? 6 : I.matrix_coeffs;
    if (cf == 1 && I.full_range_flag && m != 0 && m != 8)
      return taken(hipdec_color_420_to_rgb24(y, S.stride[0], cb, S.stride[1], cr, S.stride[2], S.width, S.height, &nclx, out_dev,
                                       out_stride, out_chroma == 11, s));
    // 4:4:4 planes take Op_YCbCr_to_RGB<uint8_t> + Op_RGB_to_RGB24_32 whatever the range (the only chain the planner has for them)
    return taken(hipdec_color_ycbcr_to_rgb24_float(y, S.stride[0], cb, S.stride[1], cr, S.stride[2], S.width, S.height,
                                             cf, &nclx, out_dev, out_stride, out_chroma == 11, s));
  }
  if (out_chroma == 12 || out_chroma == 14) {
    if (!S.wide) return set_error(HIPDEC_ERR_UNSUPPORTED, "to_rgb: RRGGBB output needs >8-bit planes");
    const int m = I.matrix_coeffs == 2 ? 6 : I.matrix_coeffs;
    if (cf != 1 || m == 0 || m == 8)     // planner rule: the 4:2:0 op does not take these; Op_YCbCr_to_RGB<uint16_t> + the interleave does
      return taken(hipdec_color_ycbcr_to_rrggbb_float(y, S.stride[0], cb, S.stride[1], cr, S.stride[2], S.width, S.height, I.bit_depth_luma,
                                                cf, &nclx, out_dev, out_stride, out_chroma == 14, s));
    return taken(hipdec_color_420_to_rrggbb(y, S.stride[0], cb, S.stride[1], cr, S.stride[2], S.width, S.height, I.bit_depth_luma,
                                      &nclx, out_dev, out_stride, out_chroma == 14, s));
  }
  return set_error(HIPDEC_ERR_UNSUPPORTED, "to_rgb: unsupported output chroma %d", out_chroma);
}

int batch_to_rgb_impl(hipdec_batch* b, int i, int out_chroma, void* out_dev, size_t out_stride, void* stream, const ScaleRequest* rq)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb: the batch's arena was handed to another batch");
  const PicParams& P = b->params[i];
  const RgbSource S{{b->arena + P.off_out[0], b->arena + P.off_out[1], b->arena + P.off_out[2]}, {P.out_stride[0], P.out_stride[1], P.out_stride[2]},
                    P.out_width, P.out_height, P.chroma_format_idc, b->wide, &b->pics[i].info, b->max_pixels};
  struct MarkDone {   // whatever is enqueued from the point the stream is resolved belongs to this batch (hipdec_batch_status / free wait for it)
    hipdec_batch* b; bool armed; hipStream_t s;
    ~MarkDone() { if (armed) b->mark_done(s ? s : default_stream()); }
  } mark{b, false, nullptr};
  return source_to_rgb(S, out_chroma, out_dev, out_stride, rq, [&]() -> void* {
    void* s = stream ? (void*)follow_stream(b, stream) : (void*)b->last_stream;
    mark.armed = true; mark.s = (hipStream_t)s;
    return s;
  });
}

// ---- orientation codes (include/heif_hipdec.h hipdec_orientation): code = r + 4 * m is "rotate counter-clockwise by r quarter turns, then mirror horizontally
// if m" - M^m R^r in the dihedral group of the square, where R M = M R^-1.  A further rotation R^k in front gives M^m R^(r + k) (m clear) or M^m R^(r - k)
// (m set); a horizontal mirror toggles m; the vertical mirror is M R^2 and so toggles m after adding a half turn.  -1: not an operation.
int orientation_compose(int o, int op, int arg)
{
  if (o < 0 || o > 7) return -1;
  const int r = o & 3, m = o >> 2;
  if (op == HIPDEC_XF_ROTATE_CCW) {
    if (arg != 90 && arg != 180 && arg != 270) return -1;
    const int k = arg / 90;
    return ((m ? r - k + 4 : r + k) & 3) + 4 * m;
  }
  if (op == HIPDEC_XF_MIRROR) {
    if (arg == 1) return r + 4 * (m ^ 1);
    if (arg == 0) return ((m ? r - 2 + 4 : r + 2) & 3) + 4 * (m ^ 1);
  }
  return -1;
}

// ---- tensor output (include/heif_hipdec.h): what hipdec_batch_to_tensor and hipdec_image_to_tensor (decoder_color_boundary.inc) share
std::atomic<uint64_t> g_tensor_calls{0}, g_tensor_entries{0};

size_t tensor_elem_bytes(int dtype) { return dtype == HIPDEC_TENSOR_U8 ? 1 : (dtype == HIPDEC_TENSOR_F32 ? 4 : 2); }

// the description's own refusals; *bytes: the size of the tensor
int tensor_check_desc(const char* who, const hipdec_tensor_desc* d, int n_entries, size_t* bytes)
{
  if (!d || n_entries < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (d->width < 1 || d->height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: output size %d x %d", who, d->width, d->height);
  if (d->dtype < HIPDEC_TENSOR_U8 || d->dtype > HIPDEC_TENSOR_BF16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown dtype %d", who, d->dtype);
  if (d->layout != HIPDEC_TENSOR_NCHW && d->layout != HIPDEC_TENSOR_NHWC) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown layout %d", who, d->layout);
  if (d->filter != HIPDEC_SCALE_NEAREST && d->filter != HIPDEC_SCALE_BOX && !resample_filter(d->filter))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown filter %d", who, d->filter);
  if (d->dtype != HIPDEC_TENSOR_U8)
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(d->scale[c]) || !std::isfinite(d->bias[c])) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: scale / bias of channel %d is not finite", who, c);
  const uint64_t per = 3ull * (uint64_t)d->width * (uint64_t)d->height * tensor_elem_bytes(d->dtype);   // (evaluated before the check below, which keeps it far from 2^64)
  if ((uint64_t)d->width * (uint64_t)d->height > (1ull << 40) || per > (~0ull) / (uint64_t)n_entries) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: tensor too large", who);
  *bytes = (size_t)(per * (uint64_t)n_entries);
  return 0;
}

// bilinear / bicubic are defined on the 8-bit picture (Pillow has no native-depth form): a float dtype from a source above 8 bits is refused
int tensor_check_resample_depth(const char* who, const hipdec_tensor_desc* d, int bits)
{
  if (resample_filter(d->filter) && bits > 8 && d->dtype != HIPDEC_TENSOR_U8)
    return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: filter %d from a %d-bit source is defined for HIPDEC_TENSOR_U8 only (the 8-bit picture is what is resampled)", who, d->filter, bits);
  return 0;
}

// the window of an entry inside a w x h picture (all zeros: the whole picture)
int tensor_window(const char* who, const hipdec_tensor_entry* e, int idx, int w, int h, int* left, int* top, int* rw, int* rh)
{
  *left = 0; *top = 0; *rw = w; *rh = h;
  if (!e || (!e->left && !e->top && !e->width && !e->height)) return 0;
  if (e->width < 1 || e->height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: window size %d x %d", who, idx, e->width, e->height);
  if (e->left < 0 || e->top < 0 || (int64_t)e->left + e->width > w || (int64_t)e->top + e->height > h)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: window %d x %d at (%d, %d) leaves the picture of %d x %d", who, idx, e->width, e->height, e->left, e->top, w, h);
  *left = e->left; *top = e->top; *rw = e->width; *rh = e->height;
  return 0;
}

// One entry: sets the tensor request and goes through the colour entry point the planner rules of hipdec_batch_to_rgb / hipdec_color_convert select for
// these planes (cf: their chroma format, 0 monochrome) - out_chroma 10 for 8-bit sources and the U8 dtype, 14 (the native-depth value) otherwise; box
// presents the planes as the 4:4:4 image they are scaled to.  The entry point records the block (color.hip); elem0: the entry's first element.
int tensor_record_entry(const char* who, const uint8_t* y, size_t ys, const uint8_t* cb, size_t cbs, const uint8_t* cr, size_t crs, int w, int h, int bits, int cf,
                        const hipdec_nclx* nclx, const hipdec_nclx* nclx_after_sdr, const hipdec_tensor_desc* d, int left, int top, int rw, int rh, int flip, void* elem0,
                        int orientation = -1, size_t pitch = 0, int plane_rows = 0, int patch = 0, int merge = 1, int tpatch = 1, bool* strided_box = nullptr,
                        const int* frame_vis = nullptr, bool composed = false)   // frame_vis: a framed entry's visible part (placed_entry), a composed entry's piece
{
  if (int rc = tensor_check_resample_depth(who, d, bits)) return rc;
  TensorRequest rq;
  memset(&rq, 0, sizeof(rq));
  rq.patch = patch; rq.merge = merge;
  rq.ow = d->width; rq.oh = d->height;
  rq.resample = resample_filter(d->filter) ? d->filter : 0;
  if (orientation < 0 && rq.resample) {   // k_resample stores through the oriented path: an unoriented entry is code 0 (the mirror with a flip) and a dense pitch
    rq.code = flip ? HIPDEC_ORIENT_MIRROR : HIPDEC_ORIENT_0;
    rq.pitch = pitch ? pitch : (size_t)d->width * (d->layout == HIPDEC_TENSOR_NHWC ? 3 : 1);
    flip = 0;
  }
  if (orientation >= 0) {   // oriented output: d->width x height is the DISPLAYED size, the kernels work on the pre-orientation picture; the flip becomes part of the code
    rq.oriented = 1;
    rq.code = flip ? orientation_compose(orientation, HIPDEC_XF_MIRROR, 1) : orientation;
    if (rq.code & 1) { rq.ow = d->height; rq.oh = d->width; }
    rq.pitch = pitch ? pitch : (size_t)d->width * (d->layout == HIPDEC_TENSOR_NHWC ? 3 : 1);
    flip = 0;
  }
  // clips (decoder_clips.inc; *strided_box in: the call may take k_clip_box, out: this entry does): a box entry whose rows stay rows in their order
  rq.tpatch = tpatch;
  if (strided_box) *strided_box = *strided_box && rq.oriented && !rq.resample && !patch && d->filter == HIPDEC_SCALE_BOX && (rq.code == HIPDEC_ORIENT_0 || rq.code == HIPDEC_ORIENT_MIRROR);
  rq.strided_box = strided_box && *strided_box;
  if (frame_vis) { rq.framed = composed ? 2 : 1; for (int k = 0; k < 4; k++) rq.frame_vis[k] = frame_vis[k]; }
  rq.plane_rows = plane_rows ? plane_rows : d->height;   // (d->height: the displayed rows)
  rq.sH = cf == 1 || cf == 2 ? 1 : 0; rq.sV = cf == 1 ? 1 : 0;
  rq.left = left; rq.top = top; rq.rw = rw; rq.rh = rh; rq.flip = flip; rq.nhwc = d->layout == HIPDEC_TENSOR_NHWC;
  for (int c = 0; c < 3; c++) { rq.scale[c] = d->scale[c]; rq.bias[c] = d->bias[c]; }
  struct Scope { ~Scope() { color_tensor_clear(); } } scope;
  color_tensor_request(rq);
  const bool wide = bits > 8;
  int rc;
  if (!cf) {   // Op_mono_to_RGB24_32: 8-bit only, as hipdec_batch_to_rgb
    if (wide) return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: monochrome input goes to 8-bit RGB only", who);
    rc = hipdec_color_mono_to_rgb24(y, ys, nullptr, 0, w, h, elem0, 0, 0, nullptr);
  } else {
    if (d->filter == HIPDEC_SCALE_BOX) cf = 3;
    const int matrix = nclx && nclx->has_nclx ? (nclx->matrix_coefficients == 2 ? 6 : nclx->matrix_coefficients) : 6;
    const int full = nclx && nclx->has_nclx ? nclx->full_range_flag : 1;
    const bool int_op = cf == 1 && full && matrix != 0 && matrix != 8;
    if (!wide) {
      rc = int_op ? hipdec_color_420_to_rgb24(y, ys, cb, cbs, cr, crs, w, h, nclx, elem0, 0, 0, nullptr)
                  : hipdec_color_ycbcr_to_rgb24_float(y, ys, cb, cbs, cr, crs, w, h, cf, nclx, elem0, 0, 0, nullptr);
    } else if (d->dtype == HIPDEC_TENSOR_U8) {
      rc = hipdec_color_hdr_to_rgb24(y, ys, cb, cbs, cr, crs, w, h, bits, cf, int_op ? nclx_after_sdr : nclx, elem0, 0, 0, int_op, nullptr);
    } else {
      rc = (cf != 1 || matrix == 0 || matrix == 8) ? hipdec_color_ycbcr_to_rrggbb_float(y, ys, cb, cbs, cr, crs, w, h, bits, cf, nclx, elem0, 0, 1, nullptr)
                                                   : hipdec_color_420_to_rrggbb(y, ys, cb, cbs, cr, crs, w, h, bits, nclx, elem0, 0, 1, nullptr);
    }
  }
  if (!rc && color_tensor_pending()) return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: the colour entry point did not take the tensor request", who);
  return rc;
}

}  // namespace

extern "C" {

size_t hipdec_tensor_bytes(const hipdec_tensor_desc* desc, int n_entries)
{
  size_t bytes = 0;
  return tensor_check_desc("tensor_bytes", desc, n_entries, &bytes) ? 0 : bytes;
}

void hipdec_tensor_stats(uint64_t* tensors, uint64_t* entries)
{
  if (tensors) *tensors = g_tensor_calls.load();
  if (entries) *entries = g_tensor_entries.load();
}

}  // extern "C"

namespace {
// the orientation list of an oriented call (NULL: all 0)
int check_orientations(const char* who, const char* what, const int* orientations, int n)
{
  for (int e = 0; orientations && e < n; e++)
    if (orientations[e] < 0 || orientations[e] > 7) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: %s %d: orientation %d is not 0 .. 7", who, what, e, orientations[e]);
  return 0;
}

// ---- placed tensor output (hipdec_batch_to_tensor_placed / hipdec_album_to_tensor_placed): what the two forms share
// framed (hipdec_batch_to_tensor_framed / hipdec_album_to_tensor_framed): a rectangle may leave the canvas, and the k_frame_* kernels store its visible part
// composed (hipdec_batch_to_tensor_composed / hipdec_album_to_tensor_composed): `composed` with tiles on n_canvases canvases in place of the rectangles
struct PlacedArgs { const hipdec_tensor_place* places; const hipdec_tensor_fill* fill; void* mask; bool framed = false;
                    bool composed = false; const hipdec_tensor_tile* tiles = nullptr; int n_canvases = 0; };
constexpr int kFrameReach = 1 << 24;   // |x|, |y| and the sides of a framed rectangle: sums and products of two stay far inside 64 bits

// what the arguments alone decide (the description has passed tensor_check_desc)
int placed_check(const char* who, const hipdec_tensor_desc* d, const PlacedArgs& pa, int n_entries)
{
  for (int e = 0; pa.places && e < n_entries; e++) {
    const hipdec_tensor_place& pl = pa.places[e];
    if (pl.width < 1 || pl.height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle size %d x %d", who, e, pl.width, pl.height);
    if (pa.framed) {
      if (pl.width > kFrameReach || pl.height > kFrameReach || pl.x > kFrameReach || pl.x < -kFrameReach || pl.y > kFrameReach || pl.y < -kFrameReach)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle %d x %d at (%d, %d): offsets and sides reach 2^24 at most", who, e, pl.width, pl.height, pl.x, pl.y);
      if ((int64_t)pl.x + pl.width <= 0 || (int64_t)pl.y + pl.height <= 0 || pl.x >= d->width || pl.y >= d->height)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle %d x %d at (%d, %d) has no pixel on the canvas of %d x %d", who, e, pl.width, pl.height, pl.x,
                         pl.y, d->width, d->height);
      hipdec_tensor_desc sample = *d;   // what the oriented call refuses for a tensor of the rectangle's size
      sample.width = pl.width; sample.height = pl.height;
      size_t bytes = 0;
      if (tensor_check_desc(who, &sample, 1, &bytes))
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle size %d x %d: the sample is too large", who, e, pl.width, pl.height);
      continue;
    }
    if (pl.x < 0 || pl.y < 0 || (int64_t)pl.x + pl.width > d->width || (int64_t)pl.y + pl.height > d->height)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle %d x %d at (%d, %d) leaves the canvas of %d x %d", who, e, pl.width, pl.height, pl.x, pl.y,
                       d->width, d->height);
  }
  if (!pa.fill) return 0;
  const hipdec_tensor_fill& f = *pa.fill;
  if (f.domain != HIPDEC_FILL_COMPONENT && f.domain != HIPDEC_FILL_ELEMENT) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown fill domain %d", who, f.domain);
  if (f.reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: fill.reserved is %d, not 0", who, f.reserved);
  for (int c = 0; c < 3; c++) {
    const float v = f.value[c];
    if (!std::isfinite(v)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: fill of channel %d is not finite", who, c);
    const bool integral = v == std::floor(v);
    if (f.domain == HIPDEC_FILL_COMPONENT) {   // (above 255 with a float dtype: held against the sources' bit depth by placed_check_component)
      if (!integral || v < 0.0f || v > (d->dtype == HIPDEC_TENSOR_U8 ? 255.0f : 65535.0f))
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: component fill %g of channel %d is not an integer a pixel can have", who, (double)v, c);
    } else if (d->dtype == HIPDEC_TENSOR_U8 && (!integral || v < 0.0f || v > 255.0f)) {
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: element fill %g of channel %d is not an integer in 0 .. 255", who, (double)v, c);
    }
  }
  return 0;
}

// a component fill against the range of the component values entry e gets: 0 .. 255, or 0 .. 2^bits - 1 for a float dtype from a source above 8 bits
int placed_check_component(const char* who, const hipdec_tensor_desc* d, const PlacedArgs& pa, int e, int bits)
{
  if (!pa.fill || pa.fill->domain != HIPDEC_FILL_COMPONENT) return 0;
  const float top = (float)((1 << (d->dtype != HIPDEC_TENSOR_U8 && bits > 8 ? bits : 8)) - 1);
  for (int c = 0; c < 3; c++)
    if (pa.fill->value[c] > top)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: component fill %g of channel %d is above %g, the largest value of its source", who, e,
                       (double)pa.fill->value[c], c, (double)top);
  return 0;
}

// entry e of a placed call: *sample is the description of the sample in its rectangle, *elem0 the rectangle's first element, *m the entry's margin block
// Framed: vis is the part of the rectangle on the canvas, in the sample's displayed coordinates (x0, y0, x1, y1); *elem0 - where the rectangle's first
// element would lie, in front of the canvas for a negative offset - is dereferenced inside it only, and the margin block names the visible rectangle.
void placed_entry(const hipdec_tensor_desc* d, const PlacedArgs& pa, int e, void* out_dev, size_t entry_bytes, hipdec_tensor_desc* sample, void** elem0, CanvasMargin* m,
                  int* vis = nullptr)
{
  const hipdec_tensor_place whole{0, 0, d->width, d->height};
  const hipdec_tensor_place& pl = pa.places ? pa.places[e] : whole;
  const size_t k = d->layout == HIPDEC_TENSOR_NHWC ? 3 : 1;
  uint8_t* canvas = (uint8_t*)out_dev + (size_t)e * entry_bytes;
  *sample = *d;
  sample->width = pl.width; sample->height = pl.height;
  *elem0 = canvas + ((int64_t)pl.y * (int64_t)d->width + (int64_t)pl.x) * (int64_t)(k * tensor_elem_bytes(d->dtype));
  const int x0 = pl.x < 0 ? -pl.x : 0, y0 = pl.y < 0 ? -pl.y : 0;   // (a placed rectangle lies on the canvas: all of it is visible)
  const int x1 = (int)std::min<int64_t>(pl.width, (int64_t)d->width - pl.x), y1 = (int)std::min<int64_t>(pl.height, (int64_t)d->height - pl.y);
  if (vis) { vis[0] = x0; vis[1] = y0; vis[2] = x1; vis[3] = y1; }
  memset(m, 0, sizeof(*m));
  m->o0 = canvas;
  m->mask = pa.mask ? (uint8_t*)pa.mask + (size_t)e * (size_t)d->width * (size_t)d->height : nullptr;
  m->W = d->width; m->H = d->height; m->x = pl.x + x0; m->y = pl.y + y0; m->w = x1 - x0; m->h = y1 - y0;
  m->nhwc = d->layout == HIPDEC_TENSOR_NHWC;
  m->domain = pa.fill ? pa.fill->domain : HIPDEC_FILL_COMPONENT;
  m->margin = m->w != d->width || m->h != d->height;
  for (int c = 0; c < 3; c++) { m->value[c] = pa.fill ? pa.fill->value[c] : 0.0f; m->scale[c] = d->scale[c]; m->bias[c] = d->bias[c]; }
}

// ---- composed tensor output (hipdec_batch_to_tensor_composed / hipdec_album_to_tensor_composed): what the two forms and hipdec_compose_visible_area share
// A rectangle in canvas coordinates, half open.
struct ComposeRect { int x0, y0, x1, y1; };
// What the tiles alone decide, per call: the pieces every entry owns and the cover table of every canvas (hipdec_internal.h CanvasCover).
struct ComposePlan {
  std::vector<std::vector<ComposeRect>> pieces;   // per entry, disjoint, in canvas coordinates; empty: the entry is fully hidden
  std::vector<int32_t> words;                     // the cover tables of all canvases
  std::vector<size_t> table;                      // per canvas: its table's first word
  std::vector<int> bands, intervals;              // per canvas
  std::vector<uint8_t> uncovered;                 // per canvas: a pixel no region covers
  uint64_t n_pieces = 0, hidden = 0;
};

// r without s: the rows of r above s, those below it, and what lies left and right of s in between - up to four disjoint rectangles, in that order
void compose_subtract(const ComposeRect& r, const ComposeRect& s, std::vector<ComposeRect>* out)
{
  if (s.x0 >= r.x1 || s.x1 <= r.x0 || s.y0 >= r.y1 || s.y1 <= r.y0) { out->push_back(r); return; }
  const int ya = std::max(r.y0, s.y0), yb = std::min(r.y1, s.y1);
  if (r.y0 < ya) out->push_back({r.x0, r.y0, r.x1, ya});
  if (yb < r.y1) out->push_back({r.x0, yb, r.x1, r.y1});
  if (r.x0 < s.x0) out->push_back({r.x0, ya, s.x0, yb});
  if (s.x1 < r.x1) out->push_back({s.x1, ya, r.x1, yb});
}

// The tiles of a call on canvases of W x H (positive): refusals name the entry; *plan is filled.  Nothing here reads a handle or touches a device.
int compose_plan(const char* who, int W, int H, const hipdec_tensor_tile* tiles, int n_entries, int n_canvases, ComposePlan* plan)
{
  if (!tiles) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: no tiles", who);
  if (n_entries < 1 || n_canvases < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: %d entries on %d canvases", who, n_entries, n_canvases);
  std::vector<ComposeRect> region((size_t)n_entries);
  std::vector<std::vector<int>> of((size_t)n_canvases);   // per canvas: its entries, ascending
  auto far = [](const hipdec_tensor_place& p) {
    return p.width > kFrameReach || p.height > kFrameReach || p.x > kFrameReach || p.x < -kFrameReach || p.y > kFrameReach || p.y < -kFrameReach;
  };
  for (int e = 0; e < n_entries; e++) {
    const hipdec_tensor_tile& t = tiles[e];
    const hipdec_tensor_place& pl = t.place;
    if (t.canvas < 0 || t.canvas >= n_canvases) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: canvas %d of %d", who, e, t.canvas, n_canvases);
    if (pl.width < 1 || pl.height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle size %d x %d", who, e, pl.width, pl.height);
    const bool whole = !t.clip.width && !t.clip.height;
    if (!whole && (t.clip.width < 1 || t.clip.height < 1))
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: clip size %d x %d (0 x 0: the whole canvas)", who, e, t.clip.width, t.clip.height);
    if (far(pl) || (!whole && far(t.clip)))
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle %d x %d at (%d, %d), clip %d x %d at (%d, %d): offsets and sides reach 2^24 at most", who, e,
                       pl.width, pl.height, pl.x, pl.y, t.clip.width, t.clip.height, t.clip.x, t.clip.y);
    ComposeRect r{std::max(pl.x, 0), std::max(pl.y, 0), std::min(pl.x + pl.width, W), std::min(pl.y + pl.height, H)};   // (below 2^25: no overflow)
    if (!whole) { r.x0 = std::max(r.x0, t.clip.x); r.y0 = std::max(r.y0, t.clip.y); r.x1 = std::min(r.x1, t.clip.x + t.clip.width); r.y1 = std::min(r.y1, t.clip.y + t.clip.height); }
    if (r.x0 >= r.x1 || r.y0 >= r.y1)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle %d x %d at (%d, %d) and its clip share no pixel of the canvas of %d x %d", who, e, pl.width,
                       pl.height, pl.x, pl.y, W, H);
    region[(size_t)e] = r;
    if (of[(size_t)t.canvas].size() == HIPDEC_COMPOSE_MAX_ENTRIES)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: canvas %d has more than %d entries", who, e, t.canvas, HIPDEC_COMPOSE_MAX_ENTRIES);
    of[(size_t)t.canvas].push_back(e);
  }
  plan->pieces.assign((size_t)n_entries, {});
  plan->table.assign((size_t)n_canvases, 0); plan->bands.assign((size_t)n_canvases, 0); plan->intervals.assign((size_t)n_canvases, 0);
  plan->uncovered.assign((size_t)n_canvases, 0);
  plan->words.clear(); plan->n_pieces = 0; plan->hidden = 0;
  std::vector<ComposeRect> cur, nxt;
  std::vector<int> edges;
  std::vector<std::pair<int, int>> spans;
  for (int cv = 0; cv < n_canvases; cv++) {
    const std::vector<int>& es = of[(size_t)cv];
    for (size_t a = 0; a < es.size(); a++) {   // pieces: the region without the regions of the later entries
      cur.assign(1, region[(size_t)es[a]]);
      for (size_t j = a + 1; j < es.size() && !cur.empty(); j++) {
        nxt.clear();
        for (const ComposeRect& r : cur) compose_subtract(r, region[(size_t)es[j]], &nxt);
        cur.swap(nxt);
        if (cur.size() > HIPDEC_COMPOSE_MAX_PIECES) break;
      }
      plan->n_pieces += cur.size();
      if (plan->n_pieces > HIPDEC_COMPOSE_MAX_PIECES)
        return set_error(HIPDEC_ERR_LIMIT, "%s: entry %d: the call has more than %d pieces", who, es[a], HIPDEC_COMPOSE_MAX_PIECES);
      if (cur.empty()) plan->hidden++;
      plan->pieces[(size_t)es[a]] = cur;
    }
    // the cover table: bands between the distinct row edges, per band the merged column intervals of the regions that cross it
    edges.assign({0, H});
    for (int e : es) { edges.push_back(region[(size_t)e].y0); edges.push_back(region[(size_t)e].y1); }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    const int nb = (int)edges.size() - 1;
    const size_t t0 = plan->words.size();
    plan->table[(size_t)cv] = t0; plan->bands[(size_t)cv] = nb;
    plan->words.resize(t0 + 2 * ((size_t)nb + 1));
    for (int k = 0; k <= nb; k++) plan->words[t0 + (size_t)k] = edges[(size_t)k];
    uint64_t covered = 0;
    int n_iv = 0;
    for (int k = 0; k < nb; k++) {
      plan->words[t0 + (size_t)nb + 1 + (size_t)k] = n_iv;
      spans.clear();
      for (int e : es) if (region[(size_t)e].y0 <= edges[(size_t)k] && edges[(size_t)k] < region[(size_t)e].y1) spans.emplace_back(region[(size_t)e].x0, region[(size_t)e].x1);
      std::sort(spans.begin(), spans.end());
      for (size_t i = 0; i < spans.size();) {
        int x0 = spans[i].first, x1 = spans[i].second;
        for (i++; i < spans.size() && spans[i].first <= x1; i++) x1 = std::max(x1, spans[i].second);   // (abutting intervals merge as well)
        plan->words.push_back(x0); plan->words.push_back(x1);
        covered += (uint64_t)(x1 - x0) * (uint64_t)(edges[(size_t)k + 1] - edges[(size_t)k]);
        n_iv++;
      }
    }
    plan->words[t0 + 2 * (size_t)nb + 1] = n_iv;
    plan->intervals[(size_t)cv] = n_iv;
    plan->uncovered[(size_t)cv] = covered < (uint64_t)W * (uint64_t)H;
    if (plan->words.size() * sizeof(int32_t) > kComposeTableBytes)
      return set_error(HIPDEC_ERR_LIMIT, "%s: the cover tables of this call exceed %zu bytes", who, (size_t)kComposeTableBytes);
  }
  return 0;
}

// a piece in the displayed coordinates of its entry's sample (x0, y0, x1, y1): the window of a framed block
void compose_piece_window(const ComposeRect& r, const hipdec_tensor_place& pl, int* vis)
{
  vis[0] = r.x0 - pl.x; vis[1] = r.y0 - pl.y; vis[2] = r.x1 - pl.x; vis[3] = r.y1 - pl.y;
}

// what the arguments of a composed call alone decide, after tensor_check_desc: the tiles, the samples' sizes, the fill
int composed_check(const char* who, const hipdec_tensor_desc* d, const PlacedArgs& pa, int n_entries, ComposePlan* plan)
{
  if (int rc = compose_plan(who, d->width, d->height, pa.tiles, n_entries, pa.n_canvases, plan)) return rc;
  for (int e = 0; e < n_entries; e++) {
    hipdec_tensor_desc sample = *d;   // what the oriented call refuses for a tensor of the rectangle's size
    sample.width = pa.tiles[e].place.width; sample.height = pa.tiles[e].place.height;
    size_t bytes = 0;
    if (tensor_check_desc(who, &sample, 1, &bytes))
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: rectangle size %d x %d: the sample is too large", who, e, sample.width, sample.height);
  }
  return placed_check(who, d, pa, n_entries);   // (no places: the fill)
}

// entry e of a composed call: *sample is the description of the sample in its rectangle, *elem0 where the rectangle's first element would lie in its canvas
void composed_entry(const hipdec_tensor_desc* d, const PlacedArgs& pa, int e, void* out_dev, size_t canvas_bytes, hipdec_tensor_desc* sample, void** elem0)
{
  const hipdec_tensor_place& pl = pa.tiles[e].place;
  const size_t k = d->layout == HIPDEC_TENSOR_NHWC ? 3 : 1;
  *sample = *d;
  sample->width = pl.width; sample->height = pl.height;
  *elem0 = (uint8_t*)out_dev + (size_t)pa.tiles[e].canvas * canvas_bytes + ((int64_t)pl.y * (int64_t)d->width + (int64_t)pl.x) * (int64_t)(k * tensor_elem_bytes(d->dtype));
}

// the fill and the masks of a composed call: ONE launch of k_compose_cover (color.hip) over the canvases' cover tables
int composed_cover(ColorBatchState& st, const hipdec_tensor_desc* d, const PlacedArgs& pa, const ComposePlan& plan, void* out_dev, size_t canvas_bytes, hipStream_t s)
{
  std::vector<CanvasCover> blocks((size_t)pa.n_canvases);
  for (int cv = 0; cv < pa.n_canvases; cv++) {
    CanvasCover& c = blocks[(size_t)cv];
    memset(&c, 0, sizeof(c));
    c.m.o0 = (uint8_t*)out_dev + (size_t)cv * canvas_bytes;
    c.m.mask = pa.mask ? (uint8_t*)pa.mask + (size_t)cv * (size_t)d->width * (size_t)d->height : nullptr;
    c.m.W = d->width; c.m.H = d->height;
    c.m.nhwc = d->layout == HIPDEC_TENSOR_NHWC;
    c.m.domain = pa.fill ? pa.fill->domain : HIPDEC_FILL_COMPONENT;
    c.m.margin = plan.uncovered[(size_t)cv];
    for (int ch = 0; ch < 3; ch++) { c.m.value[ch] = pa.fill ? pa.fill->value[ch] : 0.0f; c.m.scale[ch] = d->scale[ch]; c.m.bias[ch] = d->bias[ch]; }
    c.table = (uint64_t)plan.table[(size_t)cv]; c.n_bands = plan.bands[(size_t)cv]; c.n_intervals = plan.intervals[(size_t)cv];
  }
  return canvas_cover_launch(st, blocks.data(), pa.n_canvases, plan.words.data(), plan.words.size(), d->dtype, s);
}

// ---- packed tensor output (hipdec_batch_to_tensor_packed / hipdec_album_to_tensor_packed): what the two forms and hipdec_tensor_packed_layout share
struct PackedArgs { const hipdec_tensor_sample* samples; int patch, merge; };

int packed_check_patches(const char* who, const hipdec_tensor_patches* p)
{
  if (!p) return 0;
  if (p->patch < 0 || p->patch > 256) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: patch %d is not 0 .. 256", who, p->patch);
  if (p->merge < 1 || p->merge > 16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: merge %d is not 1 .. 16", who, p->merge);
  if (p->patch == 0 && p->merge != 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: merge %d without patches (dense samples take merge 1)", who, p->merge);
  if (p->reserved[0] || p->reserved[1]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: patches.reserved is not 0", who);
  return 0;
}

int packed_check_size(const char* who, int e, int w, int h, int patch, int merge)
{
  if (w < 1 || h < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: sample size %d x %d", who, e, w, h);
  if (patch && (w % (patch * merge) || h % (patch * merge)))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: sample size %d x %d is not a multiple of patch * merge = %d", who, e, w, h, patch * merge);
  return 0;
}

// what the arguments alone decide: the description has passed tensor_check_desc with a size of 1 x 1; *pk is filled from `patches`
int packed_check(const char* who, const hipdec_tensor_desc* d, const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, size_t out_bytes,
                 PackedArgs* pk)
{
  if (!samples) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: no samples", who);
  if (int rc = packed_check_patches(who, patches)) return rc;
  pk->samples = samples; pk->patch = patches ? patches->patch : 0; pk->merge = patches ? patches->merge : 1;
  const uint64_t room = (uint64_t)out_bytes / tensor_elem_bytes(d->dtype);
  std::vector<std::pair<uint64_t, int>> order((size_t)n_entries);
  for (int e = 0; e < n_entries; e++) {
    const hipdec_tensor_sample& sm = samples[e];
    if (int rc = packed_check_size(who, e, sm.width, sm.height, pk->patch, pk->merge)) return rc;
    const uint64_t len = 3ull * (uint64_t)sm.width * (uint64_t)sm.height;
    if (sm.offset > room || len > room - sm.offset)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: sample of %llu elements at offset %llu leaves the output of %llu elements", who, e,
                       (unsigned long long)len, (unsigned long long)sm.offset, (unsigned long long)room);
    order[(size_t)e] = std::make_pair(sm.offset, e);
  }
  std::sort(order.begin(), order.end());
  for (int k = 0; k + 1 < n_entries; k++) {
    const hipdec_tensor_sample& a = samples[order[(size_t)k].second];
    if (a.offset + 3ull * (uint64_t)a.width * (uint64_t)a.height > order[(size_t)k + 1].first)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: its elements overlap those of entry %d", who, order[(size_t)k + 1].second, order[(size_t)k].second);
  }
  return 0;
}

struct PackedSpec { const hipdec_tensor_sample* samples; const hipdec_tensor_patches* patches; };   // as the caller gave them

// entry e of a packed call: *sample is the description of the sample at its own size, *elem0 its first element
void packed_entry(const hipdec_tensor_desc* d, const PackedArgs& pk, int e, void* out_dev, hipdec_tensor_desc* sample, void** elem0)
{
  *sample = *d;
  sample->width = pk.samples[e].width; sample->height = pk.samples[e].height;
  *elem0 = (uint8_t*)out_dev + (size_t)pk.samples[e].offset * tensor_elem_bytes(d->dtype);
}

// the description of a packed call: the sizes are per sample, so its own must be 0; *unit is the copy the description's other checks see
int packed_check_desc(const char* who, const hipdec_tensor_desc* d, hipdec_tensor_desc* unit)
{
  if (!d) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (d->width || d->height) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: desc size %d x %d: the sizes are per sample, desc->width and height must be 0", who, d->width, d->height);
  *unit = *d;
  unit->width = unit->height = 1;
  return 0;
}

// hipdec_batch_to_tensor, and - oriented - hipdec_batch_to_tensor_oriented: the same checks, windows and planner rules; the oriented form records its blocks
// for the k_oriented_* kernels (color.hip) and keeps them in a parameter array of its own
// Placed (pa; always oriented): the sample goes into its rectangle of the canvas desc describes, k_canvas_margin (color.hip) writes the rest.
int batch_to_tensor_impl(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations, bool oriented, int n_entries,
                         void* out_dev, size_t out_bytes, void* stream, const PlacedArgs* pa = nullptr, const PackedSpec* ps = nullptr)
{
  if (!b || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor: bad arguments");
  size_t bytes = 0;
  hipdec_tensor_desc unit;
  PackedArgs pk{nullptr, 0, 1};
  if (ps) if (int rc = packed_check_desc("to_tensor_packed", desc, &unit)) return rc;
  const bool composed = pa && pa->composed;             // (bytes: n_canvases canvases)
  ComposePlan plan;
  if (composed && n_entries < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor_composed: %d entries", n_entries);
  if (int rc = tensor_check_desc("to_tensor", ps ? &unit : desc, composed ? pa->n_canvases : n_entries, &bytes)) return rc;
  if (oriented) if (int rc = check_orientations("to_tensor_oriented", "entry", orientations, n_entries)) return rc;
  const bool framed = pa && pa->framed && pa->places;   // (without rectangles every sample is its canvas: the oriented kernels)
  if (composed) { if (int rc = composed_check("to_tensor_composed", desc, *pa, n_entries, &plan)) return rc; }
  else if (pa) if (int rc = placed_check(pa->framed ? "to_tensor_framed" : "to_tensor_placed", desc, *pa, n_entries)) return rc;
  if (ps) { if (int rc = packed_check("to_tensor_packed", desc, ps->samples, ps->patches, n_entries, out_bytes, &pk)) return rc; }
  else if (out_bytes < bytes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor: out_bytes %zu is smaller than the tensor of %zu bytes", out_bytes, bytes);
  // (everything above is decided without reading the handle)
  if (!entries && n_entries != (int)b->pics.size())
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor: %d entries without an entry list, the batch has %d items", n_entries, (int)b->pics.size());
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor: the batch's arena was handed to another batch");
  if (!ps && b->max_pixels && (uint64_t)desc->width * (uint64_t)desc->height > b->max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "to_tensor: output of %d x %d pixels exceeds max_image_size_pixels", desc->width, desc->height);
  for (int e = 0; ps && b->max_pixels && e < n_entries; e++)
    if ((uint64_t)pk.samples[e].width * (uint64_t)pk.samples[e].height > b->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "to_tensor_packed: entry %d: sample of %d x %d pixels exceeds max_image_size_pixels", e, pk.samples[e].width, pk.samples[e].height);
  for (int e = 0; framed && b->max_pixels && e < n_entries; e++)
    if ((uint64_t)pa->places[e].width * (uint64_t)pa->places[e].height > b->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "to_tensor_framed: entry %d: rectangle of %d x %d pixels exceeds max_image_size_pixels", e, pa->places[e].width, pa->places[e].height);
  for (int e = 0; composed && b->max_pixels && e < n_entries; e++)
    if ((uint64_t)pa->tiles[e].place.width * (uint64_t)pa->tiles[e].place.height > b->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "to_tensor_composed: entry %d: rectangle of %d x %d pixels exceeds max_image_size_pixels", e, pa->tiles[e].place.width,
                       pa->tiles[e].place.height);
  return guarded("to_tensor", [&]() -> int {
    hipStream_t s = follow_stream(b, stream);
    const size_t entry_bytes = bytes / (size_t)(composed ? pa->n_canvases : n_entries);   // (composed: a canvas)
    std::vector<CanvasMargin> margins(pa && !composed ? (size_t)n_entries : 0);
    color_tensor_begin();
    for (int e = 0; e < n_entries; e++) {
      const int i = entries ? entries[e].item : e;
      if (i < 0 || i >= (int)b->pics.size()) { color_tensor_abort(); return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_tensor: entry %d names item %d of %d", e, i, (int)b->pics.size()); }
      const PicParams& P = b->params[i];
      const hipdec_image_info& I = b->pics[i].info;
      int left, top, rw, rh;
      int rc = tensor_window("to_tensor", entries ? entries + e : nullptr, e, P.out_width, P.out_height, &left, &top, &rw, &rh);
      // the decoder reports the VUI colour description exactly as the libde265 plugin would attach it (hipdec_batch_to_rgb hands it on as it is)
      hipdec_nclx nclx{1, I.colour_primaries, I.transfer_characteristics, I.matrix_coeffs, I.full_range_flag};
      hipdec_tensor_desc sample = *desc;
      void* elem0 = (uint8_t*)out_dev + (size_t)e * entry_bytes;
      size_t pitch = 0;
      int plane_rows = 0;
      int vis[4];
      if (pa) {
        if (!rc) rc = placed_check_component(composed ? "to_tensor_composed" : (pa->framed ? "to_tensor_framed" : "to_tensor_placed"), desc, *pa, e, b->wide ? I.bit_depth_luma : 8);
        if (composed) composed_entry(desc, *pa, e, out_dev, entry_bytes, &sample, &elem0);
        else placed_entry(desc, *pa, e, out_dev, entry_bytes, &sample, &elem0, &margins[(size_t)e], vis);
        pitch = (size_t)desc->width * (desc->layout == HIPDEC_TENSOR_NHWC ? 3 : 1); plane_rows = desc->height;
      }
      if (ps) packed_entry(desc, pk, e, out_dev, &sample, &elem0);   // (its own size, dense pitch and plane: the defaults of the sample's description)
      // one request; a composed entry: one per piece it owns (none when it is hidden), the piece as the window of the framed kernels
      const size_t n_req = composed ? plan.pieces[(size_t)e].size() : 1;
      if (!rc && composed) rc = tensor_check_resample_depth("to_tensor_composed", desc, b->wide ? I.bit_depth_luma : 8);   // (a hidden entry is refused as a visible one)
      for (size_t q = 0; !rc && q < n_req; q++) {
        if (composed) compose_piece_window(plan.pieces[(size_t)e][q], pa->tiles[e].place, vis);
        rc = tensor_record_entry("to_tensor", b->arena + P.off_out[0], P.out_stride[0], b->arena + P.off_out[1], P.out_stride[1], b->arena + P.off_out[2], P.out_stride[2],
                                 P.out_width, P.out_height, b->wide ? I.bit_depth_luma : 8, P.chroma_format_idc, &nclx, &nclx, &sample, left, top, rw, rh,
                                 entries ? entries[e].flip : 0, elem0, oriented ? (orientations ? orientations[e] : 0) : -1, pitch, plane_rows, pk.patch, pk.merge, 1, nullptr,
                                 framed || composed ? vis : nullptr, composed);
      }
      if (rc) { color_tensor_abort(); return rc; }
    }
    const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
    hipEvent_t* ev = b->ev.data() + kEv * slot;
    HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
    // (resampled entries are not hipdec_batch_tensor_block's blocks: they go with the oriented ones)
    int rc = color_tensor_launch(ps ? b->color_packed : (oriented || resample_filter(desc->filter) ? b->color_oriented : b->color_tensor), desc->filter, desc->dtype, s);
    if (!rc && composed) rc = composed_cover(b->color_margin, desc, *pa, plan, out_dev, entry_bytes, s);
    else if (!rc && pa) rc = canvas_margin_launch(b->color_margin, margins.data(), n_entries, desc->dtype, s);   // (disjoint elements: no order between the two but the stream's)
    HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
    if (!rc && b->runs) b->colour_timed[slot] = 1;
    b->mark_done(s);
    if (!rc) { g_tensor_calls++; g_tensor_entries += (uint64_t)n_entries; }
    if (!rc && pa && !pa->framed && !composed) placed_note_call((uint64_t)n_entries);
    if (!rc && pa && pa->framed) framed_note_call((uint64_t)n_entries);
    if (!rc && composed) composed_note_call((uint64_t)n_entries, plan.n_pieces, plan.hidden);
    if (!rc && ps) packed_note_call((uint64_t)n_entries, pk.patch > 0);
    return rc;
  });
}

// ---- the two-stage tensor forms (hipdec_batch / hipdec_album _to_tensor_warped and _to_tensor_photo): the existing resize launch writes a U8 / NHWC
// intermediate into the handle's scratch memory, a stage of color.hip reads it and writes the tensor.  A stage is what differs between the forms:
//   src_width(), src_height()   the intermediate's size
//   check(who, d, n)            what the stage's arguments alone decide
//   depth(who, d, e, bits)      the stage is defined on the 8-bit picture: a float dtype from a source above 8 bits is refused
//   scratch(b, bytes, s, out)   the intermediate, from the state the batch keeps for the stage
//   launch(b, src, d, n, out, s)
struct WarpStage {
  const hipdec_warp_desc* warp; const hipdec_tensor_map* maps; const hipdec_tensor_fill* fill;
  int src_width() const { return warp->src_width; }
  int src_height() const { return warp->src_height; }
  int check(const char* who, const hipdec_tensor_desc* d, int n) const { return warp_check(who, warp, maps, fill, d, n); }
  int depth(const char* who, const hipdec_tensor_desc* d, int e, int bits) const
  {
    if (bits > 8 && d->dtype != HIPDEC_TENSOR_U8)
      return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: entry %d: a warp from a %d-bit source is defined for HIPDEC_TENSOR_U8 only (the 8-bit picture is what is warped)", who, e, bits);
    return 0;
  }
  int scratch(hipdec_batch* b, size_t bytes, hipStream_t s, void** out) const { return warp_scratch(b->warp, bytes, s, out); }
  int launch(hipdec_batch* b, const void* src, const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s) const
  {
    return warp_launch(b->warp, src, warp, maps, fill, d, n, out_dev, s);
  }
};

struct ProjectStage {   // the warp stage with a PERSPECTIVE or QUAD map per entry; the handle's state is the warped calls'
  const hipdec_warp_desc* warp; const hipdec_tensor_projection* maps; const hipdec_tensor_fill* fill;
  int src_width() const { return warp->src_width; }
  int src_height() const { return warp->src_height; }
  int check(const char* who, const hipdec_tensor_desc* d, int n) const { return project_check(who, warp, maps, fill, d, n); }
  int depth(const char* who, const hipdec_tensor_desc* d, int e, int bits) const { return WarpStage{warp, nullptr, fill}.depth(who, d, e, bits); }
  int scratch(hipdec_batch* b, size_t bytes, hipStream_t s, void** out) const { return warp_scratch(b->warp, bytes, s, out); }
  int launch(hipdec_batch* b, const void* src, const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s) const
  {
    return project_launch(b->warp, src, warp, maps, fill, d, n, out_dev, s);
  }
};

struct PhotoStage {   // the photo stage and the augment stage: what the ChainView admits is what differs
  const hipdec_photo_desc* photo; ChainView chains;
  int src_width() const { return photo->src_width; }
  int src_height() const { return photo->src_height; }
  int check(const char* who, const hipdec_tensor_desc* d, int n) const { return chain_check(who, photo, chains, d, n); }
  int depth(const char* who, const hipdec_tensor_desc* d, int e, int bits) const
  {
    if (bits > 8 && d->dtype != HIPDEC_TENSOR_U8)
      return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: entry %d: the photometric operations on a %d-bit source are defined for HIPDEC_TENSOR_U8 only (they work on the 8-bit picture)", who, e, bits);
    return 0;
  }
  int scratch(hipdec_batch* b, size_t bytes, hipStream_t s, void** out) const { return photo_scratch(b->photo, bytes, s, out); }
  int launch(hipdec_batch* b, const void* src, const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s) const
  {
    return chain_launch(b->photo, src, photo, chains, d, n, out_dev, s);
  }
};

// What the arguments alone decide; *mid: the description of the U8 / NHWC intermediate, *mid_bytes its size
template <typename Stage>
int two_stage_check(const char* who, const Stage& stage, const hipdec_tensor_desc* desc, const int* orientations, int n_entries, const void* out_dev, size_t out_bytes,
                    hipdec_tensor_desc* mid, size_t* mid_bytes)
{
  if (!out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  size_t bytes = 0;
  if (int rc = tensor_check_desc(who, desc, n_entries, &bytes)) return rc;
  if (int rc = check_orientations(who, "entry", orientations, n_entries)) return rc;
  if (int rc = stage.check(who, desc, n_entries)) return rc;
  if (out_bytes < bytes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: out_bytes %zu is smaller than the tensor of %zu bytes", who, out_bytes, bytes);
  memset(mid, 0, sizeof(*mid));
  mid->width = stage.src_width(); mid->height = stage.src_height(); mid->dtype = HIPDEC_TENSOR_U8; mid->layout = HIPDEC_TENSOR_NHWC; mid->filter = desc->filter;
  for (int c = 0; c < 3; c++) mid->scale[c] = 1.0f;
  return tensor_check_desc(who, mid, n_entries, mid_bytes);
}

// what a two-stage form reads from its handle once the arguments alone have passed: the batch that owns the stage's state and whose stream is followed
// (an album's: its own), the items an entry can name, and the limits
struct TwoStageSource { hipdec_batch* b; int device, n_items; bool retired; uint64_t max_pixels; };

// source(): the TwoStageSource of the handle; bits(i): the bit depth of the samples item i hands to the colour stage; resize(mid, out, bytes, stream): the
// handle's oriented tensor form
template <typename Stage, typename Source, typename Bits, typename Resize>
int to_tensor_two_stage(const char* who, const void* handle, const Stage& stage, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                        int n_entries, void* out_dev, size_t out_bytes, void* stream, Source source, Bits bits, Resize resize)
{
  if (!handle) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  hipdec_tensor_desc mid;
  size_t mid_bytes = 0;
  if (int rc = two_stage_check(who, stage, desc, orientations, n_entries, out_dev, out_bytes, &mid, &mid_bytes)) return rc;
  // (everything above is decided without reading the handle)
  const TwoStageSource S = source();
  for (int e = 0; e < n_entries; e++) {
    const int i = entries ? entries[e].item : e;
    if (i < 0 || i >= S.n_items) continue;   // (the resize stage refuses it)
    if (int rc = stage.depth(who, desc, e, bits(i))) return rc;
  }
  DeviceScope scope(S.device);
  if (S.retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: the batch's arena was handed to another batch", who);
  if (S.max_pixels && (uint64_t)desc->width * (uint64_t)desc->height > S.max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "%s: output of %d x %d pixels exceeds max_image_size_pixels", who, desc->width, desc->height);
  void* scratch = nullptr;
  if (int rc = guarded(who, [&]() -> int { return stage.scratch(S.b, mid_bytes, follow_stream(S.b, stream), &scratch); })) return rc;
  if (int rc = resize(&mid, scratch, mid_bytes, stream)) return rc;   // the existing resize launch
  return guarded(who, [&]() -> int {
    hipStream_t s = follow_stream(S.b, stream);
    const int rc = stage.launch(S.b, scratch, desc, n_entries, out_dev, s);
    S.b->mark_done(s);
    return rc;
  });
}

template <typename Stage>
int batch_to_tensor_two_stage(const char* who, hipdec_batch* b, const Stage& stage, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                              int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return to_tensor_two_stage(
      who, b, stage, desc, entries, orientations, n_entries, out_dev, out_bytes, stream,
      [&]() { return TwoStageSource{b, b->device, (int)b->pics.size(), b->retired, b->max_pixels}; },
      [&](int i) { return b->wide ? b->pics[i].info.bit_depth_luma : 8; },
      [&](const hipdec_tensor_desc* mid, void* out, size_t bytes, void* st) { return batch_to_tensor_impl(b, mid, entries, orientations, true, n_entries, out, bytes, st); });
}

// what the RGB forms of the oriented output decide for one picture from the arguments alone (before a device is touched)
int rgb_oriented_check_item(const char* who, int i, int out_chroma, int code, int ow, int oh, int filter, size_t stride)
{
  if (out_chroma != 10) return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: out_chroma %d (interleaved RGB24, 10, is the oriented form)", who, out_chroma);
  if (code < 0 || code > 7) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: item %d: orientation %d is not 0 .. 7", who, i, code);
  if (ow < 1 || oh < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: item %d: output size %d x %d", who, i, ow, oh);
  if (filter != HIPDEC_SCALE_NEAREST && filter != HIPDEC_SCALE_BOX && !resample_filter(filter)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown filter %d", who, filter);
  if (stride < (size_t)ow * 3) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: item %d: out_stride %zu is smaller than a row of %zu bytes", who, i, stride, (size_t)ow * 3);
  return 0;
}

// one picture of an oriented RGB call: a U8 / NHWC entry over the whole picture whose rows are out_stride apart (code -1: the same entry for an unoriented
// call with a resampling filter, which has no other way to a row pitch)
int rgb_oriented_record(const char* who, const RgbSource& S, int code, int ow, int oh, int filter, void* out_dev, size_t out_stride)
{
  if (S.max_pixels && (uint64_t)ow * (uint64_t)oh > S.max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "%s: output of %d x %d pixels exceeds max_image_size_pixels", who, ow, oh);
  hipdec_tensor_desc d;
  memset(&d, 0, sizeof(d));
  d.width = ow; d.height = oh; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
  for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
  const hipdec_image_info& I = *S.info;
  hipdec_nclx nclx{1, I.colour_primaries, I.transfer_characteristics, I.matrix_coeffs, I.full_range_flag};
  return tensor_record_entry(who, S.plane[0], S.stride[0], S.plane[1], S.stride[1], S.plane[2], S.stride[2], S.width, S.height, S.wide ? I.bit_depth_luma : 8,
                             S.chroma_format_idc, &nclx, &nclx, &d, 0, 0, S.width, S.height, 0, out_dev, code, out_stride);
}

// hipdec_batch_to_rgb_scaled (item `first`) and hipdec_batch_to_rgb_scaled_all (all items) with a resampling filter: the pictures as U8 / NHWC entries whose
// rows are out_stride apart, ONE launch of k_resample.  Interleaved RGB24 only; what the arguments alone decide is refused before the batch is looked at.
int batch_rgb_resample(const char* who, hipdec_batch* b, int first, bool all, int out_chroma, const int* ows, const int* ohs, int filter, void* const* outs,
                       const size_t* strides, void* stream)
{
  if (out_chroma != 10) return set_error(HIPDEC_ERR_UNSUPPORTED, "%s: out_chroma %d with filter %d (bilinear / bicubic write interleaved RGB24, out_chroma 10)", who, out_chroma, filter);
  if (!b || !ows || !ohs || !outs || !strides || (!all && (first < 0 || first >= (int)b->pics.size()))) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  const int n = all ? (int)b->pics.size() : 1;
  for (int i = 0; i < n; i++) {
    if (!outs[i]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: item %d: no output", who, first + i);
    if (int rc = rgb_oriented_check_item(who, first + i, out_chroma, 0, ows[i], ohs[i], filter, strides[i])) return rc;
  }
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: the batch's arena was handed to another batch", who);
  return guarded(who, [&]() -> int {
    hipStream_t s = follow_stream(b, stream);
    color_tensor_begin();
    for (int i = 0; i < n; i++) {
      const PicParams& P = b->params[first + i];
      const RgbSource S{{b->arena + P.off_out[0], b->arena + P.off_out[1], b->arena + P.off_out[2]}, {P.out_stride[0], P.out_stride[1], P.out_stride[2]},
                        P.out_width, P.out_height, P.chroma_format_idc, b->wide, &b->pics[first + i].info, b->max_pixels};
      if (int rc = rgb_oriented_record(who, S, -1, ows[i], ohs[i], filter, outs[i], strides[i])) { color_tensor_abort(); return rc; }
    }
    const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
    hipEvent_t* ev = b->ev.data() + kEv * slot;
    if (all) HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
    int rc = color_tensor_launch(b->color_oriented, filter, HIPDEC_TENSOR_U8, s);
    if (all) {
      HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
      if (!rc && b->runs) b->colour_timed[slot] = 1;
    }
    b->mark_done(s);
    return rc;
  });
}
}  // namespace

extern "C" {

int hipdec_orientation_compose(int orientation, int op, int arg)
{
  const int c = orientation_compose(orientation, op, arg);
  if (c < 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "orientation_compose: orientation %d, op %d, arg %d", orientation, op, arg), -1;
  return c;
}

// EXIF 1 .. 8: identity, mirror horizontal, half turn, mirror vertical, transpose, quarter turn clockwise, anti-transpose, quarter turn counter-clockwise
int hipdec_orientation_from_exif(int exif)
{
  static const int code[8] = {0, 4, 2, 6, 7, 3, 5, 1};
  if (exif < 1 || exif > 8) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "orientation_from_exif: %d is not 1 .. 8", exif), -1;
  return code[exif - 1];
}

int hipdec_batch_to_tensor(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, int n_entries, void* out_dev, size_t out_bytes,
                           void* stream)
{
  return batch_to_tensor_impl(b, desc, entries, nullptr, false, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_oriented(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations, int n_entries,
                                    void* out_dev, size_t out_bytes, void* stream)
{
  return batch_to_tensor_impl(b, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_placed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev, size_t out_bytes,
                                  void* stream)
{
  const PlacedArgs pa{places, fill, mask_dev};
  return batch_to_tensor_impl(b, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_batch_to_tensor_framed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev, size_t out_bytes,
                                  void* stream)
{
  const PlacedArgs pa{places, fill, mask_dev, true};
  return batch_to_tensor_impl(b, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_batch_to_tensor_composed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                    const hipdec_tensor_tile* tiles, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, int n_canvases, void* out_dev,
                                    size_t out_bytes, void* stream)
{
  const PlacedArgs pa{nullptr, fill, mask_dev, false, true, tiles, n_canvases};
  return batch_to_tensor_impl(b, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_batch_to_tensor_warped(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_warp_desc* warp, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, int n_entries, void* out_dev,
                                  size_t out_bytes, void* stream)
{
  return batch_to_tensor_two_stage("to_tensor_warped", b, WarpStage{warp, maps, fill}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_projected(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                     const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill, int n_entries, void* out_dev,
                                     size_t out_bytes, void* stream)
{
  return batch_to_tensor_two_stage("to_tensor_projected", b, ProjectStage{warp, maps, fill}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_photo(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                 const hipdec_photo_desc* photo, const hipdec_photo_chain* chains, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return batch_to_tensor_two_stage("to_tensor_photo", b, PhotoStage{photo, chain_view(chains)}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_augmented(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                     const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return batch_to_tensor_two_stage("to_tensor_augmented", b, PhotoStage{photo, chain_view(chains)}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_batch_to_tensor_recipe(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, const hipdec_recipe_affine* affines, int n_affines,
                                  int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return batch_to_tensor_two_stage("to_tensor_recipe", b, PhotoStage{photo, recipe_view(chains, affines, n_affines)}, desc, entries, orientations, n_entries, out_dev,
                                   out_bytes, stream);
}

int hipdec_batch_to_tensor_packed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  const PackedSpec ps{samples, patches};
  return batch_to_tensor_impl(b, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, nullptr, &ps);
}

int hipdec_tensor_packed_layout(const hipdec_tensor_patches* patches, const int* widths, const int* heights, int n, uint64_t* offsets, uint32_t* tokens,
                                uint64_t* total_elements)
{
  if (!widths || !heights || n < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_packed_layout: bad arguments"), -1;
  if (packed_check_patches("tensor_packed_layout", patches)) return -1;
  const int patch = patches ? patches->patch : 0, merge = patches ? patches->merge : 1;
  uint64_t at = 0;
  for (int e = 0; e < n; e++) {
    if (packed_check_size("tensor_packed_layout", e, widths[e], heights[e], patch, merge)) return -1;
    const uint64_t len = 3ull * (uint64_t)widths[e] * (uint64_t)heights[e];
    const uint64_t tok = patch ? (uint64_t)(widths[e] / patch) * (uint64_t)(heights[e] / patch) : 0;
    if (tok > 0xffffffffull || len > ~0ull - at) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_packed_layout: entry %d: the sequence is too long", e), -1;
    if (offsets) offsets[e] = at;
    if (tokens) tokens[e] = (uint32_t)tok;
    at += len;
  }
  if (total_elements) *total_elements = at;
  return 0;
}

int hipdec_letterbox_place(int src_width, int src_height, int canvas_width, int canvas_height, int upscale, int anchor, hipdec_tensor_place* out)
{
  if (!out || src_width < 1 || src_height < 1 || canvas_width < 1 || canvas_height < 1)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "letterbox_place: source %d x %d into canvas %d x %d", src_width, src_height, canvas_width, canvas_height), -1;
  if (anchor != 0 && anchor != 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "letterbox_place: anchor %d (0 top-left, 1 centred)", anchor), -1;
  const int64_t sw = src_width, sh = src_height, cw = canvas_width, ch = canvas_height;
  int64_t w, h;
  if (!upscale && sw <= cw && sh <= ch) { w = sw; h = sh; }
  else if (sw * ch >= sh * cw) { w = cw; h = (sh * cw + sw / 2) / sw; h = h < 1 ? 1 : h; }
  else { h = ch; w = (sw * ch + sh / 2) / sh; w = w < 1 ? 1 : w; }
  out->width = (int)w; out->height = (int)h;
  out->x = anchor ? (int)((cw - w) / 2) : 0;
  out->y = anchor ? (int)((ch - h) / 2) : 0;
  return 0;
}

// torchvision's Resize(int) on the displayed size, then CenterCrop: Python's round() is round half to even, and a side shorter than the crop is padded
// with floor(d / 2) in front
int hipdec_resize_crop_place(int src_width, int src_height, int resize, int crop_width, int crop_height, hipdec_tensor_place* out)
{
  if (!out || src_width < 1 || src_height < 1 || resize < 1 || crop_width < 1 || crop_height < 1)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resize_crop_place: source %d x %d, resize %d, crop %d x %d", src_width, src_height, resize, crop_width, crop_height), -1;
  const int64_t sw = src_width, sh = src_height, r = resize;
  const int64_t w = sw <= sh ? r : r * sw / sh, h = sw <= sh ? r * sh / sw : r;
  if (w > kFrameReach || h > kFrameReach || crop_width > kFrameReach || crop_height > kFrameReach)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resize_crop_place: resized sample %lld x %lld, crop %d x %d: sides reach 2^24 at most", (long long)w, (long long)h, crop_width,
                     crop_height), -1;
  auto offset = [](int64_t side, int64_t crop) -> int {
    if (side < crop) return (int)((crop - side) / 2);
    const int64_t d = side - crop, k = d / 2;
    return (int)-(d & 1 ? k + (k & 1) : k);   // d / 2 = k + 1 / 2 goes to the even one of k and k + 1
  };
  out->x = offset(w, crop_width); out->y = offset(h, crop_height);
  out->width = (int)w; out->height = (int)h;
  return 0;
}

// the pixels every entry of a composed call owns: the areas of its pieces
int hipdec_compose_visible_area(int width, int height, const hipdec_tensor_tile* tiles, int n_entries, int n_canvases, uint64_t* area)
{
  if (!area || width < 1 || height < 1 || width > kFrameReach || height > kFrameReach)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "compose_visible_area: canvas %d x %d", width, height), -1;
  return guarded("compose_visible_area", [&]() -> int {
    ComposePlan plan;
    if (compose_plan("compose_visible_area", width, height, tiles, n_entries, n_canvases, &plan)) return -1;
    for (int e = 0; e < n_entries; e++) {
      uint64_t a = 0;
      for (const ComposeRect& r : plan.pieces[(size_t)e]) a += (uint64_t)(r.x1 - r.x0) * (uint64_t)(r.y1 - r.y0);
      area[e] = a;
    }
    return 0;
  }) ? -1 : 0;
}

// YOLOv5's mosaic-4: the four samples meet at the centre, each clipped to its quadrant
int hipdec_mosaic_tiles(int canvas_w, int canvas_h, int xc, int yc, const int* widths, const int* heights, int canvas, hipdec_tensor_tile* out)
{
  if (!out || !widths || !heights || canvas < 0 || canvas_w < 1 || canvas_h < 1 || canvas_w > kFrameReach || canvas_h > kFrameReach || xc <= 0 || xc >= canvas_w ||
      yc <= 0 || yc >= canvas_h)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "mosaic_tiles: canvas %d of %d x %d, centre (%d, %d)", canvas, canvas_w, canvas_h, xc, yc), -1;
  for (int k = 0; k < 4; k++)
    if (widths[k] < 1 || heights[k] < 1 || widths[k] > kFrameReach || heights[k] > kFrameReach)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "mosaic_tiles: sample %d of %d x %d (1 .. 2^24 each way)", k, widths[k], heights[k]), -1;
  for (int k = 0; k < 4; k++) {
    const bool right = k & 1, low = k >> 1;
    out[k].canvas = canvas;
    out[k].place = hipdec_tensor_place{right ? xc : xc - widths[k], low ? yc : yc - heights[k], widths[k], heights[k]};
    out[k].clip = hipdec_tensor_place{right ? xc : 0, low ? yc : 0, right ? canvas_w - xc : xc, low ? canvas_h - yc : yc};
  }
  return 0;
}

// a contact sheet: entry k letterboxed (centred) into cell k, row-major
int hipdec_sheet_tiles(int cols, int rows, int cell_w, int cell_h, int gap, const int* widths, const int* heights, int n, int upscale, int canvas, hipdec_tensor_tile* out)
{
  if (!out || !widths || !heights || canvas < 0 || cols < 1 || rows < 1 || cell_w < 1 || cell_h < 1 || gap < 0 || n < 1 || (int64_t)n > (int64_t)cols * rows)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "sheet_tiles: %d samples in %d x %d cells of %d x %d, gap %d, canvas %d", n, cols, rows, cell_w, cell_h, gap, canvas), -1;
  const int64_t sheet_w = (int64_t)cols * cell_w + (int64_t)(cols - 1) * gap, sheet_h = (int64_t)rows * cell_h + (int64_t)(rows - 1) * gap;
  if (sheet_w > kFrameReach || sheet_h > kFrameReach)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "sheet_tiles: a sheet of %lld x %lld: sides reach 2^24 at most", (long long)sheet_w, (long long)sheet_h), -1;
  for (int k = 0; k < n; k++) {
    const int64_t cx = (int64_t)(k % cols) * ((int64_t)cell_w + gap), cy = (int64_t)(k / cols) * ((int64_t)cell_h + gap);
    hipdec_tensor_place pl;
    if (hipdec_letterbox_place(widths[k], heights[k], cell_w, cell_h, upscale, 1, &pl)) return -1;   // (its message stands)
    out[k].canvas = canvas;
    out[k].place = hipdec_tensor_place{(int)(cx + pl.x), (int)(cy + pl.y), pl.width, pl.height};
    out[k].clip = hipdec_tensor_place{(int)cx, (int)cy, cell_w, cell_h};
  }
  return 0;
}

int hipdec_batch_to_rgb_scaled_oriented_all(hipdec_batch* b, int out_chroma, const int* orientations, const int* out_widths, const int* out_heights, int filter,
                                            void* const* outs_dev, const size_t* out_strides, void* stream)
{
  const char* who = "to_rgb_scaled_oriented_all";
  if (!b || !out_widths || !out_heights || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  const int n = (int)b->pics.size();
  for (int i = 0; i < n; i++) {
    if (!outs_dev[i]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: item %d: no output", who, i);
    if (int rc = rgb_oriented_check_item(who, i, out_chroma, orientations ? orientations[i] : 0, out_widths[i], out_heights[i], filter, out_strides[i])) return rc;
  }
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: the batch's arena was handed to another batch", who);
  return guarded(who, [&]() -> int {
    hipStream_t s = follow_stream(b, stream);
    color_tensor_begin();
    for (int i = 0; i < n; i++) {
      const PicParams& P = b->params[i];
      const RgbSource S{{b->arena + P.off_out[0], b->arena + P.off_out[1], b->arena + P.off_out[2]}, {P.out_stride[0], P.out_stride[1], P.out_stride[2]},
                        P.out_width, P.out_height, P.chroma_format_idc, b->wide, &b->pics[i].info, b->max_pixels};
      if (int rc = rgb_oriented_record(who, S, orientations ? orientations[i] : 0, out_widths[i], out_heights[i], filter, outs_dev[i], out_strides[i])) { color_tensor_abort(); return rc; }
    }
    const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
    hipEvent_t* ev = b->ev.data() + kEv * slot;
    HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
    int rc = color_tensor_launch(b->color_oriented, filter, HIPDEC_TENSOR_U8, s);
    HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
    if (!rc && b->runs) b->colour_timed[slot] = 1;
    b->mark_done(s);
    return rc;
  });
}

int hipdec_batch_tensor_block(hipdec_batch* b, int entry, int plane, const void** plane_dev, size_t* plane_stride, int* x, int* y, int* width, int* height)
{
  if (!b || !plane_dev || !plane_stride || !x || !y || !width || !height) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_block: bad arguments");
  return color_tensor_inspect(b->color_tensor, entry, plane, plane_dev, plane_stride, x, y, width, height);
}

int hipdec_batch_to_rgb(hipdec_batch* b, int i, int out_chroma, void* out_dev, size_t out_stride, void* stream)
{
  return batch_to_rgb_impl(b, i, out_chroma, out_dev, out_stride, stream, nullptr);
}

int hipdec_batch_to_rgb_scaled(hipdec_batch* b, int i, int out_chroma, int out_width, int out_height, int filter, void* out_dev, size_t out_stride, void* stream)
{
  if (resample_filter(filter)) return batch_rgb_resample("to_rgb_scaled", b, i, false, out_chroma, &out_width, &out_height, filter, &out_dev, &out_stride, stream);
  const ScaleRequest rq{out_width, out_height, filter};
  return batch_to_rgb_impl(b, i, out_chroma, out_dev, out_stride, stream, &rq);
}

int hipdec_batch_to_rgb_scaled_all(hipdec_batch* b, int out_chroma, const int* out_widths, const int* out_heights, int filter, void* const* outs_dev,
                                   const size_t* out_strides, void* stream)
{
  if (resample_filter(filter)) return batch_rgb_resample("to_rgb_scaled_all", b, 0, true, out_chroma, out_widths, out_heights, filter, outs_dev, out_strides, stream);
  if (!b || !out_widths || !out_heights || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb_scaled_all: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb_scaled_all: the batch's arena was handed to another batch");
  hipStream_t s = follow_stream(b, stream);
  color_capture_begin();
  for (int i = 0; i < (int)b->pics.size(); i++) {
    const ScaleRequest rq{out_widths[i], out_heights[i], filter};
    if (int rc = batch_to_rgb_impl(b, i, out_chroma, outs_dev[i], out_strides[i], (void*)s, &rq)) { color_capture_abort(); return rc; }
  }
  const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
  hipEvent_t* ev = b->ev.data() + kEv * slot;
  HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
  int rc = color_capture_launch_scaled(b->color_scaled, filter, s);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
  if (!rc && b->runs) b->colour_timed[slot] = 1;
  b->mark_done(s);
  return rc;
}

// plane c of item i through the plane scaler into a host buffer: what hipdec_image_scale hands out for that plane
int hipdec_batch_read_plane_scaled(hipdec_batch* b, int i, int c, int out_width, int out_height, int filter, void* dst, size_t dst_stride)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || c < 0 || c > 2 || !dst) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: the batch's arena was handed to another batch");
  if (out_width < 1 || out_height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: output size %d x %d", out_width, out_height);
  if (filter != HIPDEC_SCALE_NEAREST && filter != HIPDEC_SCALE_BOX) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: unknown filter %d", filter);
  if (b->max_pixels && (uint64_t)out_width * (uint64_t)out_height > b->max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "read_plane_scaled: output of %d x %d pixels exceeds max_image_size_pixels", out_width, out_height);
  const PicParams& P = b->params[i];
  if (c > 0 && !P.chroma_format_idc) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: monochrome image has no chroma planes");
  const size_t es = b->wide ? 2 : 1;
  const int sx = c && P.chroma_format_idc != 3 ? 2 : 1, sy = c && P.chroma_format_idc == 1 ? 2 : 1;
  const int qw = (out_width + sx - 1) / sx, qh = (out_height + sy - 1) / sy;
  if (dst_stride < (size_t)qw * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_plane_scaled: dst_stride %zu is smaller than a row of %zu bytes", dst_stride, (size_t)qw * es);
  return guarded("read_plane_scaled", [&]() -> int {
    hipStream_t s = follow_stream(b, nullptr);
    const size_t st = ((size_t)qw * es + 255) & ~(size_t)255;
    void* d = nullptr; size_t cap = 0;
    HIPDEC_CHECK_HIP(arena_acquire(&d, st * (size_t)qh + 256, &cap));
    struct Release { hipStream_t s; void* d; size_t cap; ~Release() { (void)hipStreamSynchronize(s); arena_release(d, cap); } } rel{s, d, cap};
    uint8_t* rows = (uint8_t*)d + 256;   // (the parameter block in front of the rows)
    PlaneScaleParams j{b->arena + P.off_out[c], P.out_stride[c], c ? P.out_cwidth : P.out_width, c ? P.out_cheight : P.out_height, rows, st, qw, qh,
                       P.out_width, P.out_height, out_width, out_height, 0};
    static_assert(sizeof(PlaneScaleParams) <= 256, "parameter block");
    int rc = scale_planes_launch(&j, 1, (int)es, filter, d, s);
    b->mark_done(s);
    if (rc) return rc;
    return copy_rows_to_host(dst, dst_stride, rows, st, (size_t)qw * es, qh, s);
  });
}

int hipdec_batch_to_rgb_all(hipdec_batch* b, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream)
{
  if (!b || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb_all: bad arguments");
  DeviceScope scope(b->device);
  hipStream_t s = follow_stream(b, stream);
  // every item goes through the per-item entry point (argument checks, planner rule, coefficients) in capture mode
  color_capture_begin();
  for (int i = 0; i < (int)b->pics.size(); i++)
    if (int rc = hipdec_batch_to_rgb(b, i, out_chroma, outs_dev[i], out_strides[i], (void*)s)) { color_capture_abort(); return rc; }
  // device time of the colour stage goes into the timing slot of the decode run it follows
  const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
  hipEvent_t* ev = b->ev.data() + kEv * slot;
  HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
  int rc = color_capture_launch(b->color, s);
  HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
  if (!rc && b->runs) b->colour_timed[slot] = 1;
  b->mark_done(s);
  return rc;
}

// decode + colour stage of every item as ONE call: for 8-bit 4:2:0 batches going to interleaved RGB24 the colour conversion is fused into
// the SAO kernel's store path (planes are still written: the ABI hands them out); every other case runs the decode kernels followed by the
// batched colour kernel, exactly like hipdec_batch_run + hipdec_batch_to_rgb_all.
int hipdec_batch_run_rgb(hipdec_batch* b, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream)
{
  if (!b || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "run_rgb: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "run_rgb: the batch's arena was handed to another batch");
  if (int rc = ensure_init()) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  static const bool no_fusion = getenv("HIPDEC_NO_SAO_RGB_FUSION") != nullptr;
  bool fuse = out_chroma == 10 && !b->wide && !no_fusion;
  for (const auto& P : b->params) fuse = fuse && P.chroma_format_idc == 1;
  if (!fuse) {
    if (int rc = hipdec_batch_run(b, stream)) return rc;
    return hipdec_batch_to_rgb_all(b, out_chroma, outs_dev, out_strides, nullptr);
  }
  // the per-item entry points check the arguments, apply the planner rule and fill the coefficient blocks (capture mode: nothing is launched)
  hipStream_t ps = stage_overlap() ? post_stream() : s;
  color_capture_begin();
  for (int i = 0; i < (int)b->pics.size(); i++)
    if (int rc = hipdec_batch_to_rgb(b, i, out_chroma, outs_dev[i], out_strides[i], (void*)ps)) { color_capture_abort(); return rc; }
  const void* dev = nullptr;
  int variant = -1, count = 0;
  if (int rc = color_capture_take(b->color, ps, &dev, &variant, &count)) return rc;
  if (variant != color_variant_rgb24_u8() || count != (int)b->pics.size()) return set_error(HIPDEC_ERR_UNSUPPORTED, "run_rgb: unexpected colour variant");
  b->last_stream = s;
  b->ran = true;
  b->fused_rgb = true;
  return launch_all(*b, s, dev);
}

int hipdec_batch_timing_slots(hipdec_batch* b, int slots)
{
  if (!b || slots < 1 || slots > 4096) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "timing_slots: bad arguments");
  DeviceScope scope(b->device);
  if (b->ran) HIPDEC_CHECK_HIP(b->wait());
  for (auto& e : b->ev) if (e) (void)hipEventDestroy(e);
  b->ev.assign((size_t)slots * kEv, nullptr);
  b->colour_timed.assign((size_t)slots, 0);
  for (auto& e : b->ev) HIPDEC_CHECK_HIP(hipEventCreate(&e));
  b->runs = 0; b->ran = false;
  return 0;
}

int hipdec_batch_slot_kernel_timing_us(hipdec_batch* b, int slot, float out[8])
{
  if (!b || !out || slot < 0 || (size_t)slot >= b->ev.size() / kEv || (uint64_t)slot >= b->runs)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "slot_timing: no run recorded in slot %d", slot);
  DeviceScope scope(b->device);
  hipEvent_t* ev = b->ev.data() + kEv * (size_t)slot;
  HIPDEC_CHECK_HIP(hipEventSynchronize(ev[5]));
  for (int k = 0; k < 5; k++) {
    float ms = 0;
    HIPDEC_CHECK_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
    out[k] = ms * 1000.0f;
  }
  out[5] = 0.0f;
  if (b->colour_timed[(size_t)slot]) {
    float ms = 0;
    HIPDEC_CHECK_HIP(hipEventSynchronize(ev[7]));
    HIPDEC_CHECK_HIP(hipEventElapsedTime(&ms, ev[6], ev[7]));
    out[5] = ms * 1000.0f;
  }
  float ms = 0;
  HIPDEC_CHECK_HIP(hipEventElapsedTime(&ms, ev[0], ev[5]));
  out[6] = ms * 1000.0f;
  out[7] = 0.0f;
  return 0;
}

int hipdec_batch_slot_timing_us(hipdec_batch* b, int slot, float out[5])
{
  float k[8];
  if (int rc = hipdec_batch_slot_kernel_timing_us(b, slot, k)) return rc;
  out[0] = k[0]; out[1] = k[1] + k[2]; out[2] = k[3]; out[3] = k[4]; out[4] = k[6];
  return 0;
}

int hipdec_batch_last_timing_us(hipdec_batch* b, float out[5])
{
  if (!b || !b->ran || !out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "last_timing: batch has not been run");
  return hipdec_batch_slot_timing_us(b, (int)((b->runs - 1) % (b->ev.size() / kEv)), out);
}

int hipdec_batch_read_tap(hipdec_batch* b, int i, int which, int c, void* dst, size_t dst_stride)
{
  if (!b || i < 0 || i >= (int)b->pics.size() || c < 0 || c > 2 || !dst) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_tap: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_tap: the batch's arena was handed to another batch");
  (void)which;  // the reconstruction buffer holds the deblocked picture after a full run
  const PicParams& P = b->params[i];
  return copy_plane_d2h(*b, P.off_rec[c], P.rec_stride[c], c ? P.cwidth : P.width, c ? P.cheight : P.height, dst, dst_stride);
}

int hipdec_batch_read_maps(hipdec_batch* b, int i, uint8_t* log2_tb, uint8_t* log2_cb, uint8_t* intra_luma, uint8_t* intra_chroma, int8_t* qp_y,
                           uint8_t* flags, size_t map_elems)
{
  if (!b || i < 0 || i >= (int)b->pics.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_maps: bad arguments");
  DeviceScope scope(b->device);
  if (b->retired) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_maps: the batch's arena was handed to another batch");
  const PicParams& P = b->params[i];
  const int uw = (P.width + 3) / 4, uh = (P.height + 3) / 4;
  if (map_elems < (size_t)uw * uh) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "read_maps: buffers too small");
  const size_t nunits = ((size_t)P.ctb_w * P.ctb_h) << P.units_per_ctb_log2;
  std::vector<uint8_t> sz(nunits), fl(nunits), ipm(nunits), ipmc(nunits), qp(nunits);
  HIPDEC_CHECK_HIP(hipMemcpy(sz.data(), b->arena + P.off_u_size, nunits, hipMemcpyDeviceToHost));
  HIPDEC_CHECK_HIP(hipMemcpy(fl.data(), b->arena + P.off_u_flags, nunits, hipMemcpyDeviceToHost));
  HIPDEC_CHECK_HIP(hipMemcpy(ipm.data(), b->arena + P.off_u_ipm, nunits, hipMemcpyDeviceToHost));
  HIPDEC_CHECK_HIP(hipMemcpy(ipmc.data(), b->arena + P.off_u_ipmc, nunits, hipMemcpyDeviceToHost));
  HIPDEC_CHECK_HIP(hipMemcpy(qp.data(), b->arena + P.off_u_qp, nunits, hipMemcpyDeviceToHost));
  const int l = P.log2_ctb - 2, mask = (1 << l) - 1;
  auto il = [](uint32_t x, uint32_t y) {
    x = (x | (x << 2)) & 0x33; x = (x | (x << 1)) & 0x55; y = (y | (y << 2)) & 0x33; y = (y | (y << 1)) & 0x55; return x | (y << 1);
  };
  for (int uy = 0; uy < uh; uy++)
    for (int ux = 0; ux < uw; ux++) {
      const size_t idx = (((size_t)(uy >> l) * P.ctb_w + (ux >> l)) << P.units_per_ctb_log2) + il(ux & mask, uy & mask);
      const size_t o = (size_t)uy * uw + ux;
      if (log2_tb) log2_tb[o] = sz[idx] & 15;
      if (log2_cb) log2_cb[o] = sz[idx] >> 4;
      if (intra_luma) intra_luma[o] = ipm[idx] & 63;
      if (intra_chroma) intra_chroma[o] = ipmc[idx];
      if (qp_y) qp_y[o] = (int8_t)qp[idx];
      if (flags) flags[o] = fl[idx];
    }
  return 0;
}

int hipdec_probe(const void* data, size_t size, uint64_t max_image_size_pixels, hipdec_image_info* info)
{
  if (!data || !info) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "probe: bad arguments");
  return guarded("probe", [&]() -> int {
    ParsedPicture pp;
    std::string err;
    int rc = parse_picture((const uint8_t*)data, size, max_image_size_pixels, pp, err);
    if (rc != HIPDEC_OK) return set_error(rc, "%s", err.c_str());
    *info = pp.info;
    return 0;
  });
}


}  // extern "C"

// The rest of this translation unit, by subject (one 2600-line file held five subsystems):
#include "decoder_object.inc"          // the decoder object of the plugin life cycle + the still-image coalescer
#include "decoder_chains.inc"          // look-ahead chains of sequence tracks, DPB / output order
#include "decoder_color_boundary.inc"  // resident planes, colour planner, hipdec_color_convert, image transforms
#include "decoder_grid.inc"            // grid photos over the node's GPUs
#include "decoder_album.inc"           // albums of grid photos: one launch set, one fused paste
#include "decoder_clips.inc"           // clips: the samples of several sequence tracks as one launch set, video tensors
