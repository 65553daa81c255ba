// hipdec_internal.h — internal glue shared by the host side of libheifhip.so
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <new>
#include <exception>
#include "heif_hipdec.h"

namespace hipdec {

int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int ensure_init();
// The device hipdec_init() selected — or, inside a DeviceScope on this thread, the scope's device: arenas, streams and launches of a
// multi-device grid decode (grid.hip) are created under the scope of the shard's device.
int active_device();
class DeviceScope {
 public:
  explicit DeviceScope(int device);
  ~DeviceScope();
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
 private:
  int prev_;
};
hipStream_t default_stream();
hipStream_t post_stream();      // everything behind the CABAC kernel when stage overlap is on (hipdec_set_stage_overlap)
bool stage_overlap();
int max_devices();              // size of the per-device stream table: device indices beyond it are refused
hipStream_t upload_stream();    // H2D copies of large batches (overlaps the kernels of the batch before)
uint32_t parse_wave_budget();   // CABAC pool waves one batch may launch (wave slots / concurrent batches)

// Process-wide pool of decode arenas.  libheif creates and destroys one plugin decoder per item and per grid tile
// (libheif/codecs/decoder.cc:388-405,549), so arenas are recycled by size instead of hipMalloc / hipFree per image.
hipError_t arena_acquire(void** out, size_t bytes, size_t* capacity);
void arena_release(void* p, size_t capacity);
void arena_pool_clear();
bool arena_oom_take();   // did an arena_acquire of this thread fail since the last call?  (clears the mark: a chain that ran out of device memory is retried shorter)
void set_memory_pressure_handler(void (*fn)());   // called when a device allocation fails even with the arena pool empty, before the last retry
hipError_t pinned_acquire(void** out, size_t bytes, size_t* capacity);   // pinned host staging for large uploads, recycled
void pinned_release(void* p, size_t capacity);
void pinned_pool_clear();
int32_t* status_slot_acquire();                 // pinned 64-byte slot for a batch's status word (NULL: none left)
void status_slot_release(int32_t* p);

// A small pool of HIP streams: concurrent plugin decoder instances (libheif decodes grid tiles on several threads,
// libheif/image-items/grid.cc:436) each run on their own stream so that their kernels overlap on the GPU.
hipStream_t stream_acquire();
hipStream_t stream_acquire_priority();   // for image-level calls beside the decoder's launch sets (released with stream_release)
void stream_release(hipStream_t s);

// the stream follow-up work of a batch goes on (made to wait for the batch's last recorded work when that ran elsewhere: decoder.hip follow_stream)
}  // namespace hipdec
struct hipdec_batch;
namespace hipdec {
hipStream_t batch_follow_stream(hipdec_batch* b, hipStream_t s);

// Colour stage of a whole batch as ONE launch (color.hip): between begin and launch this thread's hipdec_color_* calls record
// their parameter blocks instead of launching; the blocks live in a device array owned by the batch.
struct ColorBatchState {
  void* dev = nullptr;
  size_t dev_bytes = 0;
  std::vector<uint8_t> host;   // the blocks last uploaded
  std::vector<uint8_t> prev;   // the upload before: kept alive while a copy from it may still be pending (pageable source of an async copy)
};
void color_capture_begin();
void color_capture_abort();
int color_capture_launch(ColorBatchState& st, hipStream_t s);
int color_capture_take(ColorBatchState& st, hipStream_t s, const void** dev, int* uniform_variant, int* count);   // upload only
int color_variant_rgb24_u8();
void color_batch_state_free(ColorBatchState& st);

// Scaled output (color.hip).  A scale request set on this thread makes the NEXT hipdec_color_* entry point that ends in an interleaved layout run (or,
// in capture mode, record) the fused scale + colour kernel instead of the full-size one: argument checks, planner rules and coefficients stay theirs.
// The launch clears the request; color_scale_pending() afterwards means the entry point did not take it (the caller refuses).
// sH / sV: subsampling shifts of the chroma planes that are handed in (the box filter presents them to the entry points as 4:4:4).
void color_scale_request(int out_width, int out_height, int filter, int sH, int sV);
void color_scale_clear();
bool color_scale_pending();
int color_capture_launch_scaled(ColorBatchState& st, int filter, hipStream_t s);   // the recorded scaled blocks of this thread as ONE launch
// one plane through the plane scaler; (pw, ph) -> (qw, qh) are the PLANE's sizes, (iw, ih) -> (ow, oh) the image's (what the nearest-neighbour index uses)
struct PlaneScaleParams {
  const uint8_t* in; size_t is; int pw, ph;
  uint8_t* out; size_t os; int qw, qh;
  int iw, ih, ow, oh;
  int tile;   // box: output samples per workgroup (filled in by scale_planes_launch)
};
// n planes as one launch; dev_params: room for n blocks in device memory, `jobs` must stay alive until `s` has passed the upload
int scale_planes_launch(PlaneScaleParams* jobs, int n, int bytes_per_sample, int filter, void* dev_params, hipStream_t s);

// Tensor output (color.hip).  As a scale request: the NEXT hipdec_color_* entry point that ends in interleaved RGB24 (8-bit value) or little-endian RRGGBB
// (native-depth value) records a tensor block instead of launching - its `out` is the entry's first element - and color_tensor_launch() sends the recorded
// blocks out as ONE launch.  The window is in luma samples of the planes handed in; sH / sV are their chroma shifts (box presents them as 4:4:4).
// Oriented output: `oriented` sends the block to the k_oriented_* kernels - ow x oh is then the PRE-orientation size, `code` the hipdec_orientation with the
// entry's flip folded in, `pitch` the elements from one displayed row to the next, `plane_rows` the rows of a channel plane (NCHW: the plane is
// plane_rows * pitch elements; a dense sample: its displayed rows, a placed one: the canvas' rows).
// Packed output, patch sequences: `patch` > 0 sends the (oriented) block to the k_patch_* kernels, which store the sample as tokens of patch x patch pixels in
// groups of merge x merge (hipdec_batch_to_tensor_packed); pitch and plane_rows are then not read.
struct TensorRequest { int ow, oh, sH, sV, left, top, rw, rh, flip, nhwc; float scale[3], bias[3]; int oriented, code; size_t pitch; int plane_rows;
                       int resample; /* HIPDEC_SCALE_BILINEAR / _BICUBIC: the block is recorded for k_resample, code and pitch set for every entry (0: no) */
                       int patch, merge;
                       int tpatch;        /* clips (hipdec_clips_to_tensor_packed): frames per token, a token is 3 * tpatch * patch * patch elements (0 / 1: a still's) */
                       int strided_box;   /* clips: a box entry whose folded code is 0 or 4 goes to k_clip_box - k_tensor_box's stage, the oriented store - not k_oriented_box */
                       int framed;        /* the (oriented) block goes to the k_frame_* kernels, which store inside frame_vis only (FrameWindow below);
                                             2: a piece of a composed call - the same block, its pieces of work are not hipdec_framed_stats' */
                       int frame_vis[4]; };
// Framed tensor output (color.hip k_frame_*, include/heif_hipdec.h hipdec_batch_to_tensor_framed): the part of an entry's sample that lies on its canvas.
// A request with `framed` set carries the window in displayed coordinates of the sample (frame_vis: x0, y0, x1, y1, half open, not empty); its `out` is
// where element (0, 0, 0) of the whole sample WOULD lie - in front of the canvas where the rectangle starts above or left of it - and is dereferenced inside
// the window only.  The block the kernels read holds the window twice: as displayed columns and rows (what a store is tested against) and as columns and
// rows of the pre-orientation picture P (what a workgroup's tile, band and box rows are tested against); color.hip derives the second from the code,
// and shrinks the grid to the pieces of work between the first and the last that hold a visible pixel.
struct FrameWindow {
  int vx0, vy0, vx1, vy1;   // displayed sample
  int px0, py0, px1, py1;   // P
  int tx0, ty0;             // the first piece of work along either axis that holds a visible pixel - a column tile and a block of rows / a band of P, or the
                            // nearest kernel's 256 x 4 displayed pixels: the grid covers the pieces from there on, a workgroup adds the origin to its index
  int reserved[2];
};
void color_tensor_request(const TensorRequest& r);
void color_tensor_clear();
bool color_tensor_pending();
void color_tensor_begin();
void color_tensor_abort();
int color_tensor_launch(ColorBatchState& st, int filter, int dtype, hipStream_t s);
int color_tensor_inspect(const ColorBatchState& st, int entry, int plane, const void** plane_dev, size_t* stride, int* x, int* y, int* w, int* h);

// Placed tensor output (color.hip k_canvas_margin): everything of an entry's canvas outside its rectangle, and its mask, for all entries in ONE launch.
// One block per entry; the kernel computes the fill elements itself (tensor_elem<DT> / the RNE narrowing), so they cannot differ from a pixel's.
struct CanvasMargin {
  uint8_t* o0;             // the canvas' first element
  uint8_t* mask;           // the entry's W * H mask bytes, or NULL
  int W, H;                // the canvas
  int x, y, w, h;          // the rectangle
  int nhwc;
  int domain;              // hipdec_fill_domain
  int margin;              // the rectangle is not the whole canvas
  int reserved;
  float value[3], scale[3], bias[3];
};
// launches when an entry has a margin or a mask (nothing otherwise); dtype: hipdec_tensor_dtype
int canvas_margin_launch(ColorBatchState& st, const CanvasMargin* blocks, int n, int dtype, hipStream_t s);
// Composed tensor output (color.hip k_compose_cover, include/heif_hipdec.h hipdec_batch_to_tensor_composed): several entries share a canvas, and everything
// no entry's region covers - the fill element and the mask - goes out in ONE launch for all canvases of a call.  One block per canvas: `m` is the margin
// block of the placed call without its rectangle (o0, mask, W, H, nhwc, domain, value, scale, bias; margin: the canvas has a pixel no region covers), and
// the covered pixels are the canvas' COVER TABLE of n_bands row bands, int32 words behind the blocks in the same upload:
//   edge[0 .. n_bands]        ascending rows, edge[0] = 0 and edge[n_bands] = H: band b is the rows edge[b] .. edge[b + 1] - 1
//   first[0 .. n_bands]       band b's intervals are first[b] .. first[b + 1] - 1
//   x0, x1 per interval       the covered columns x0 .. x1 - 1 of the band: sorted, disjoint, and merged (x1 of one is below x0 of the next)
// `table` is the table's first word: the host records its index among the call's words, canvas_cover_launch turns it into the device address.
struct CanvasCover {
  CanvasMargin m;
  uint64_t table;
  int n_bands, n_intervals;
};
constexpr size_t kComposeTableBytes = 1u << 20;   // the cover tables of one call (HIPDEC_COMPOSE_TABLE_BYTES)
// launches when a canvas has an uncovered pixel or a mask (nothing otherwise); words: the tables of all canvases
int canvas_cover_launch(ColorBatchState& st, const CanvasCover* blocks, int n, const int32_t* words, size_t n_words, int dtype, hipStream_t s);
void composed_note_call(uint64_t entries, uint64_t pieces, uint64_t hidden);   // hipdec_composed_stats
void placed_note_call(uint64_t entries);   // hipdec_placed_stats
void framed_note_call(uint64_t entries);   // hipdec_framed_stats (its tile counts: the launches of the k_frame_* kernels, color.hip)
void packed_note_call(uint64_t entries, bool patches);   // hipdec_packed_stats
uint64_t clip_box_entries();   // entries that have gone through k_clip_box (hipdec_clips_stats)

// Warped tensor output (color.hip k_warp, include/heif_hipdec.h hipdec_tensor_warp): n dense U8 / NHWC samples through one affine map each, ONE launch.
// What the arguments alone decide (warp_check) is host-only; warp_launch builds the per-entry table - the six doubles, or Pillow's fixed-point values,
// or the running-sum index tables of its scale path - uploads it with one copy and launches.
struct WarpState {             // the device memory a handle (or, for hipdec_tensor_warp, the process) keeps for its warped calls
  ColorBatchState table;       // the per-entry table last uploaded
  void* scratch = nullptr;     // the U8 / NHWC intermediate of the decode-side forms
  size_t scratch_bytes = 0;
  hipEvent_t done = nullptr;   // behind the last launch that read either
  hipStream_t last = nullptr;
};
int warp_check(const char* who, const hipdec_warp_desc* w, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, const hipdec_tensor_desc* d, int n);
int warp_scratch(WarpState& st, size_t bytes, hipStream_t s, void** out);   // the handle's intermediate, at least `bytes` long
int warp_launch(WarpState& st, const void* src_dev, const hipdec_warp_desc* w, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill,
                const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s);
void warp_state_free(WarpState& st);
// Projective tensor output (color.hip k_project, include/heif_hipdec.h hipdec_tensor_project): the warped output's structure with a PERSPECTIVE or QUAD map per
// entry.  project_check is host-only; project_launch uploads n records with one copy and launches once.  The state is a WarpState - a handle's is the one its
// warped calls use (table, intermediate, event).
int project_check(const char* who, const hipdec_warp_desc* w, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill, const hipdec_tensor_desc* d, int n);
int project_launch(WarpState& st, const void* src_dev, const hipdec_warp_desc* w, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill,
                   const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s);

// Photometric tensor output (color.hip k_photo_hist / k_photo_apply, include/heif_hipdec.h hipdec_tensor_photo): n dense U8 / NHWC samples through a chain
// of up to four operations each.  What the arguments alone decide (chain_check) is host-only; chain_launch builds one table of records per chain step,
// uploads them with one copy and launches at most one histogram and one apply kernel per step.
struct PhotoState {            // the device memory a handle (or, for hipdec_tensor_photo, the process) keeps for its photo calls
  WarpState base;              // the tables last uploaded, the U8 / NHWC intermediate of the decode-side forms, the event behind the last launch
  void* work = nullptr;        // up to two ping-pong buffers of n samples, then the histograms of one step
  size_t work_bytes = 0;
};
int photo_scratch(PhotoState& st, size_t bytes, hipStream_t s, void** out);   // the handle's intermediate, at least `bytes` long
void photo_state_free(PhotoState& st);

// Augmented tensor output (color.hip k_augment_hue / k_augment_blur beside the photo kernels, include/heif_hipdec.h hipdec_tensor_augment): the photo stage
// with hue, Gaussian blur and chains of up to eight.  The same host code serves both: a ChainView reads either chain array, and per step the records are
// compacted per kind - apply, histogram, hue, blur - with at most one launch each.  The state, the scratch and the work memory are a PhotoState.
struct ChainView {             // hipdec_photo_chain and hipdec_augment_chain share their head: n_ops, reserved, ops[]
  const void* base; size_t stride; int max_ops; bool augment;
  bool recipe = false;         // the recipe surface (hipdec_tensor_recipe): the augment view plus HIPDEC_RECIPE_AFFINE steps into affines[0 .. n_affines)
  const hipdec_recipe_affine* affines = nullptr; int n_affines = 0;
  const uint8_t* at(int e) const { return (const uint8_t*)base + (size_t)e * stride; }
  int n_ops(int e) const { return ((const int*)at(e))[0]; }
  int reserved(int e) const { return ((const int*)at(e))[1]; }
  const hipdec_photo_op& op(int e, int k) const { return ((const hipdec_photo_op*)(at(e) + offsetof(hipdec_photo_chain, ops)))[k]; }   // (k below max_ops)
};
static_assert(offsetof(hipdec_photo_chain, ops) == offsetof(hipdec_augment_chain, ops) && offsetof(hipdec_photo_chain, n_ops) == 0 &&
              offsetof(hipdec_augment_chain, n_ops) == 0 && offsetof(hipdec_photo_chain, reserved) == 4 && offsetof(hipdec_augment_chain, reserved) == 4,
              "ChainView reads both chain types through their common head");
inline ChainView chain_view(const hipdec_photo_chain* c) { return ChainView{c, sizeof(hipdec_photo_chain), HIPDEC_PHOTO_MAX_OPS, false}; }
inline ChainView chain_view(const hipdec_augment_chain* c) { return ChainView{c, sizeof(hipdec_augment_chain), HIPDEC_AUGMENT_MAX_OPS, true}; }
// Recipe tensor output (color.hip k_recipe_affine_* beside the photo and augment kernels, include/heif_hipdec.h hipdec_tensor_recipe): the augment stage
// with affine steps - three more kinds of record per step, one per warp filter, each a WarpEntry whose `reserved` word is the `last` flag.
static_assert(sizeof(hipdec_recipe_affine) == 64 && offsetof(hipdec_recipe_affine, filter) == 48 && offsetof(hipdec_recipe_affine, fill) == 52,
              "hipdec_recipe_affine has no padding");
inline ChainView recipe_view(const hipdec_augment_chain* c, const hipdec_recipe_affine* affines, int n_affines)
{
  return ChainView{c, sizeof(hipdec_augment_chain), HIPDEC_AUGMENT_MAX_OPS, true, true, affines, n_affines};
}
int chain_check(const char* who, const hipdec_photo_desc* p, const ChainView& chains, const hipdec_tensor_desc* d, int n);
int chain_launch(PhotoState& st, const void* src_dev, const hipdec_photo_desc* p, const ChainView& chains, const hipdec_tensor_desc* d, int n, void* out_dev,
                 hipStream_t s);

// The paste of an album of grid photos (transform.hip k_album_paste): one job per (tile, plane), already clipped to the photo's output size by the host
// (a job clipped to nothing is not emitted); the job table lives in device memory and all jobs go out as ONE launch.
struct PasteJob {
  const uint8_t* src; uint64_t src_stride;
  uint8_t* dst; uint64_t dst_stride;
  uint32_t width_bytes, rows;
};
int album_paste_launch(const PasteJob* jobs_dev, int n_jobs, uint32_t max_rows, hipStream_t s);

// No C++ exception may cross the C ABI (the caller is libheif, or cgo / JNI / ctypes): every entry point that parses untrusted
// input or allocates runs its body through guarded().
template <class F> int guarded(const char* what, F&& body)
{
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return set_error(HIPDEC_ERR_MEMORY, "%s: out of host memory", what);
  } catch (const std::exception& e) {
    return set_error(HIPDEC_ERR_BITSTREAM, "%s: %s", what, e.what());
  } catch (...) {
    return set_error(HIPDEC_ERR_BITSTREAM, "%s: unknown failure", what);
  }
}

#define HIPDEC_CHECK_HIP(expr)                                                                  \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return hipdec::set_error(HIPDEC_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

}  // namespace hipdec
