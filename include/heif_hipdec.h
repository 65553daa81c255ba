/*
 * heif_hipdec.h — C ABI of the MI355X-native HEIC decode path (libheif_amd/libheifhip.so).
 *
 * This is the drop-in boundary below libheif's decoder-plugin layer: plain C, pointers and sizes
 * only, no torch / C++ types.  Two groups of entry points:
 *
 *  1. hipdec_decoder_*  — one instance per coded image, the same life cycle libheif drives through
 *     heif_decoder_plugin (libheif/api/libheif/heif_plugin.h:85-169; call order in
 *     libheif/codecs/decoder.cc:355-563):
 *        new_decoder2 -> push_data2 (xN) -> flush_data -> decode_next_image2 -> free_decoder
 *     and it replaces what libheif/plugins/decoder_libde265.cc does with libde265
 *     (push: :322-368, decode: :386-457, plane hand-over: :97-171, VUI colour -> nclx: :426-449).
 *     hipdec_batch_* decodes many independent items (grid tiles, batches of stills) in one set of
 *     kernel launches — the device-side form of libheif/image-items/grid.cc:405-453.
 *
 *  2. hipdec_color_* — the fused colour stage over planes resident in HBM; each entry point
 *     restates one ColorConversionOperation of libheif/color-conversion (file:line at each
 *     declaration) bit-exactly (integer ops) or with identical float arithmetic (FMA contraction
 *     off).
 *
 * All `stride` arguments are in BYTES.  Device pointers are HIP device pointers of the device
 * selected with hipdec_init().  `stream` is a hipStream_t cast to void* (NULL = the library's
 * default stream).  Every function returns 0 on success or a negative hipdec_status; a
 * thread-local message is available from hipdec_last_error().
 */
#ifndef HEIF_HIPDEC_H
#define HEIF_HIPDEC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define HIPDEC_API __attribute__((visibility("default")))
#else
#define HIPDEC_API
#endif

typedef enum hipdec_status {
  HIPDEC_OK = 0,
  HIPDEC_ERR_INVALID_ARGUMENT = -1,
  HIPDEC_ERR_END_OF_DATA = -2,       /* truncated NAL framing (heif_suberror_End_of_data)          */
  HIPDEC_ERR_BITSTREAM = -3,         /* malformed / non-conformant HEVC syntax                     */
  HIPDEC_ERR_UNSUPPORTED = -4,       /* valid HEVC outside the implemented tool set                */
  HIPDEC_ERR_LIMIT = -5,             /* security limit exceeded (max_image_size_pixels)            */
  HIPDEC_ERR_DEVICE = -6,            /* HIP runtime error / no device / kernel fault               */
  HIPDEC_ERR_NO_IMAGE = -7,          /* nothing decodable was pushed                               */
  HIPDEC_ERR_DECODE = -8,            /* device-side decode error (substream desynchronised ...)    */
  HIPDEC_ERR_MEMORY = -9             /* host allocation failed (heif_error_Memory_allocation_error) */
} hipdec_status;

/* ---- library ---------------------------------------------------------------------------------- */
HIPDEC_API int hipdec_init(int device_index);          /* idempotent; selects the device            */
HIPDEC_API void hipdec_shutdown(void);                  /* gives pools, streams and the resident-plane registry back; call it when no other thread is inside the
                                                          * library and no object of it is alive - a later call re-initialises the library by itself */
HIPDEC_API const char* hipdec_last_error(void);        /* thread-local, never NULL                  */
HIPDEC_API const char* hipdec_version(void);
HIPDEC_API int hipdec_device_count(void);

/* small device-memory helpers so that callers without a HIP toolchain (ctypes, cgo, JNI) can stage
 * buffers; real integrations pass their own device pointers */
HIPDEC_API void* hipdec_malloc(size_t bytes);
HIPDEC_API void hipdec_free(void* dptr);
HIPDEC_API int hipdec_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
HIPDEC_API int hipdec_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
HIPDEC_API int hipdec_memset(void* dst_dev, int value, size_t bytes);
HIPDEC_API int hipdec_stream_synchronize(void* stream);
/* additional HIP streams (hipStream_t as void*) so that independent batches overlap: the CABAC kernel keeps the
 * scalar pipes busy while another batch's reconstruction / filters / colour stage use the vector pipes and HBM */
HIPDEC_API void* hipdec_stream_create(void);
HIPDEC_API void hipdec_stream_destroy(void* stream);

/* ---- decoder ---------------------------------------------------------------------------------- */
typedef struct hipdec_decoder hipdec_decoder;

typedef struct hipdec_image_info {
  int width, height;              /* luma size after the conformance-window crop (== ispe)        */
  int chroma_format_idc;          /* 0 = 4:0:0, 1 = 4:2:0  (== heif_chroma numeric value)          */
  int chroma_width, chroma_height;
  int bit_depth_luma, bit_depth_chroma;
  /* VUI colour description as libde265 reports it (decoder_libde265.cc:426-449); H.265 Annex E
     defaults (2,2,2,limited) when absent */
  int colour_primaries, transfer_characteristics, matrix_coeffs, full_range_flag;
  int coded_width, coded_height;  /* pic_width/height_in_luma_samples                              */
  size_t bitstream_bytes;
  int num_substreams;             /* independent CABAC substreams (slices x tiles / WPP rows)      */
} hipdec_image_info;

/* new_decoder2 (heif_plugin.h:158; decoder_libde265.cc:175-214).  max_image_size_pixels == 0
 * means "no limit" (heif_security_limits.max_image_size_pixels, enforced before allocation as
 * decoder_libde265.cc:183-199 does). */
HIPDEC_API int hipdec_decoder_new(hipdec_decoder** out, int strict_decoding, uint64_t max_image_size_pixels);
HIPDEC_API void hipdec_decoder_free(hipdec_decoder* dec);
HIPDEC_API void hipdec_decoder_set_strict(hipdec_decoder* dec, int strict_decoding);

/* push_data2 (heif_plugin.h:160; decoder_libde265.cc:322-368): `data` is a concatenation of
 * [4-byte big-endian length][NAL unit without start code]; parameter sets first.  May be called
 * several times; the bytes are copied.  A push AFTER a decode starts the next picture (the samples of an intra-only image sequence,
 * libheif/sequences/track_visual.cc:200-280): the parameter sets seen so far stay active, so later samples may carry slice data only. */
HIPDEC_API int hipdec_decoder_push_data(hipdec_decoder* dec, const void* data, size_t size);

/* decode_next_image2 (heif_plugin.h:164; decoder_libde265.cc:386-457): parses the headers on the
 * host, runs the HIP decode pipeline and leaves the planes in HBM.  Returns HIPDEC_ERR_NO_IMAGE
 * when no picture was pushed (libheif sees "no image yet"). */
HIPDEC_API int hipdec_decoder_decode(hipdec_decoder* dec, hipdec_image_info* info);
/* The same with OUTPUT ORDER (de265_get_next_picture behind decoder_libde265.cc:402-419): decodes the pushed sample if one is pending, then
 * releases the next picture in output (POC) order when the bumping process of C.5.2.2 allows it - more pictures of the coded video sequence
 * are waiting than sps_max_num_reorder_pics, a new coded video sequence has started, or `flush` (the host's flush_data: end of the data).
 * *have = 0: no picture yet (libheif pushes the next sample).  Afterwards hipdec_decoder_read_plane* / _device_plane serve the released
 * picture.  Streams without B pictures come out in coding order, one picture per sample.  user_data: what hipdec_decoder_set_user_data
 * attached to the sample the picture was decoded from (push_data2's user_data, decoder_libde265.cc:360). */
HIPDEC_API void hipdec_decoder_set_user_data(hipdec_decoder* dec, uintptr_t user_data);
/* Look-ahead of sequence tracks: behind a decoder's first picture, hipdec_decoder_next_picture() decodes the pushed samples once `samples` of them
 * wait (or the host flushed): ONE launch set parses all of them (CABAC parsing needs nothing of a neighbour picture), the pixel stages follow picture
 * by picture in decoding order.  Until then it reports *have = 0 and libheif pushes the next sample (sequences/track_visual.cc:200-260).
 * 0 / 1: every sample is decoded at the poll behind its push.  Default 32 (environment: HIPDEC_SEQ_LOOKAHEAD; measured on 720p IPPP tracks: 19 fps without, 138 with 16, 205 with 32 samples); at most 64.  Stills are not affected:
 * the first picture of a decoder is always decoded at once. */
HIPDEC_API void hipdec_set_sequence_lookahead(int samples);
/* Pipelined chains: with `chains` > 1 a look-ahead chain is only ENQUEUED when its window is full, and its pictures are held back until `chains` of
 * them are in flight (or the host flushes) - libheif keeps pushing samples while no picture comes out (sequences/track_visual.cc:200-260), so the next
 * window fills while the chain runs and its CABAC launch (one WPP critical path, whatever the number of pictures) runs beside the pixel steps of the
 * chains in front of it.  The first picture of a chain in flight that goes out is preceded by the look at that chain's status; a chain that fails on
 * the device is undone together with the chains built on it and decoded again the plain way, so the sample that is to blame gets the error.
 * 1: every chain is waited for where it is launched.  Default 3 (environment: HIPDEC_SEQ_PIPELINE; at most 8; measured on 720p tracks, look-ahead 32: one IPPP
 * track 267 fps with 1, 550 with 3; 16 tracks side by side 1706 / 3093).  A host that wants a track's pictures with the least delay sets 1 (and a small look-ahead):
 * with D chains of L samples, up to D x L samples are pushed before the first of their pictures comes out.  Look-ahead 0 / 1 switches the pipeline off. */
HIPDEC_API void hipdec_set_sequence_pipeline(int chains);
/* statistics: chains that were left in flight when they were enqueued, and how often a failed one was undone */
HIPDEC_API void hipdec_decoder_pipeline_stats(uint64_t* chains_left_in_flight, uint64_t* rollbacks);
HIPDEC_API int hipdec_decoder_next_picture(hipdec_decoder* dec, int flush, hipdec_image_info* info, int* have, uintptr_t* user_data);
/* Concurrent hipdec_decoder_decode() calls (libheif decodes the tiles of a 'grid' item on worker threads,
 * libheif/image-items/grid.cc:405-453, one decoder instance per tile) are coalesced into shared launch sets; a
 * serial host never waits.  HIPDEC_COALESCE_WINDOW_US (default 2000, 0 = off) bounds the gathering time.
 * Counters since load: decode requests, launch sets issued, requests that shared a launch set with others. */
HIPDEC_API void hipdec_decoder_coalesce_stats(uint64_t* requests, uint64_t* launch_sets, uint64_t* shared_requests);
/* The same for sequence tracks decoded side by side (one decoder instance and one host thread per track, as libheif's Track_Visual objects,
 * libheif/sequences/track_visual.cc:200-280, are): the look-ahead chains (hipdec_set_sequence_lookahead) of instances that ask within
 * HIPDEC_CHAIN_WINDOW_US (default 20000; 0 = every chain on its own) of each other run as ONE launch set - step k of the set holds the k-th
 * dependency step of every track.  A leader only waits for instances that took part in a chain during the last second; a lone track never waits.
 * Counters since load: chains asked for, launch sets issued for them, launch sets that held more than one track's chain. */
HIPDEC_API void hipdec_decoder_chain_stats(uint64_t* chains, uint64_t* launch_sets, uint64_t* shared_launch_sets);

/* Host-only header probe: parses the parameter sets and slice segment headers of one pushed item
 * and fills `info` without touching the GPU (what libheif's own SPS pre-check does in
 * libheif/codecs/hevc_dec.cc:54-77, extended to the whole front end).  Same error codes as decode. */
HIPDEC_API int hipdec_probe(const void* data, size_t size, uint64_t max_image_size_pixels, hipdec_image_info* info);
/* For hosts that register plugins statically: heif_register_decoder_plugin(hipdec_get_decoder_plugin())
 * (libheif/api/libheif/heif_library.cc:70-81).  Returns a const heif_decoder_plugin*. */
HIPDEC_API const void* hipdec_get_decoder_plugin(void);

/* plane hand-over (decoder_libde265.cc:97-171): copies plane c (0 = Y, 1 = Cb, 2 = Cr) into a host
 * buffer with the caller's stride; samples are uint8 for bit depth 8, little-endian uint16
 * above.  A stride below the row length is refused (HIPDEC_ERR_INVALID_ARGUMENT: the last row would end past a buffer of
 * height x stride bytes); the same holds for every call that writes rows into a caller's buffer (hipdec_batch_read_plane,
 * hipdec_grid_read_plane, hipdec_batch_to_rgb, hipdec_color_convert, hipdec_grid_to_rgb). */
HIPDEC_API int hipdec_decoder_read_plane(hipdec_decoder* dec, int c, void* dst_host, size_t dst_stride);
/* the same, and remembers (host pointer -> device copy) so that hipdec_color_convert() on those very host planes skips the upload:
 * what the libheif plugin uses */
HIPDEC_API int hipdec_decoder_read_plane_tracked(hipdec_decoder* dec, int c, void* dst_host, size_t dst_stride);
/* Plane tracking on / off (default off; HIPDEC_TRACK_PLANES=1 in the environment turns it on).  While it is on,
 * hipdec_decoder_read_plane_tracked() records a hash over EVERY byte of the plane it copied out, so that a later
 * hipdec_color_convert() on the same host pointer can read the decoder's device copy instead of uploading — but only if the host
 * bytes are still exactly those (libheif edits planes in place between decode and conversion: image_item.cc:969 mirror_inplace).
 * An entry serves one conversion.  The plugin switches tracking on when the hosting libheif registers the HIP colour op
 * (INTEGRATION.md §4); the first hipdec_color_convert() call switches it on as well. */
HIPDEC_API void hipdec_set_plane_tracking(int on);
/* on = 2: for a host that ANNOUNCES every in-place edit of a handed-over plane with hipdec_forget_plane() before the colour conversion (the patched
 * libheif of libheif_amd/integration: image_item.cc:958-1004 mirror_inplace is its only one, and only as the fall-back of the device transform).  The
 * identity check then reads every 16th row instead of every byte (round 5: 38 ms of hashing per heif_decode_image() call under 256 threads). */
HIPDEC_API void hipdec_forget_plane(const void* host_plane);
/* drops every remembered (host pointer -> device copy) pair and with them the decode arenas they keep alive; hipdec_shutdown() and the
 * plugin's deinit_plugin() call it */
HIPDEC_API void hipdec_forget_resident_planes(void);
/* device-resident hand-over for callers that keep the colour stage on the GPU */
HIPDEC_API int hipdec_decoder_device_plane(hipdec_decoder* dec, int c, const void** dptr, size_t* stride);

/* Device arenas and pinned staging buffers of retired batches are parked for reuse up to this many bytes (default: a third of the
 * device's memory, single arenas up to two ninths of it - 96 / 64 GiB on an MI355X; pinned host buffers: an eighth of the host's RAM, at
 * most 24 GiB; HIPDEC_ARENA_CACHE_GIB overrides the device figure at hipdec_init): hipFree() synchronises the device, and the decoder
 * path builds one batch per launch set of concurrently decoding instances.  A host that wants the memory back lowers it; 0 empties the
 * cache. */
HIPDEC_API int hipdec_set_arena_cache_bytes(size_t bytes);

/* Two-stage pipeline across batches (default off): hipdec_batch_run() keeps the CABAC kernel on the caller's stream and queues residual /
 * reconstruction / deblock / SAO — and whatever follows for that batch: colour stage, packs — on a second stream of the device.  A host
 * that alternates two batches (two arenas) then has batch k+1's CABAC parse, which is issue- and dependency-bound, running beside batch k's
 * pixel stages.  hipdec_batch_status() / free wait for the batch as before. */
HIPDEC_API int hipdec_set_stage_overlap(int on);

/* Number of large batches the host keeps in flight at a time on separate streams (default 1).  The CABAC work pool of a
 * batch needs all its waves resident, so concurrent batches share the device's wave slots. */
HIPDEC_API int hipdec_set_concurrent_batches(int n);

/* Wave slots per SIMD (0 .. 4, default 0) the CABAC work pools leave free.  The pool's waves are resident for a whole launch set, so a host
 * that runs image-level kernels beside decoding - libheif with the colour / transformation hooks: the plugin sets 1 when it announces them -
 * keeps room for those, at 2 - 3 % of the parse rate; HIPDEC_RESERVED_WAVE_SLOTS overrides. */
HIPDEC_API int hipdec_set_reserved_wave_slots(int per_simd);

/* ---- batch decode (grid tiles / throughput mode) ------------------------------------------- */
typedef struct hipdec_batch hipdec_batch;
/* Parses n independent items (same framing as push_data; host worker threads for large batches) and uploads them; all
 * items must share chroma format and bit depth.  Large batches are staged in pinned memory and uploaded ASYNCHRONOUSLY on the
 * library's upload stream: the call returns when the host work is done, hipdec_batch_run() orders itself behind the copy, so
 * creating batch k+1 overlaps the kernels of batch k ("from compressed bytes in host memory").  `data` may be
 * released when the call returns.  hipdec_batch_run() is the device-resident hot path: inputs in HBM when it starts, decoded
 * planes in HBM when it (asynchronously) ends. */
HIPDEC_API int hipdec_batch_create(hipdec_batch** out, int n, const void* const* data, const size_t* sizes,
                                   uint64_t max_image_size_pixels);
/* The same for a stream of batches of one shape: the new batch takes over `recycle`'s arena (when it is large enough; `recycle`
 * may be NULL) and its upload is ordered behind whatever `recycle` still has in flight — decode, colour stage, packs.  One arena
 * then serves the whole stream while the host work of batch k+1 (header parsing, staging) overlaps the kernels of batch k.  After
 * the call `recycle` only answers hipdec_batch_status / timing queries and hipdec_batch_free: its planes are gone, so consume
 * them (hipdec_batch_to_rgb_all, hipdec_batch_pack_item) before creating the successor. */
HIPDEC_API int hipdec_batch_create_recycling(hipdec_batch** out, int n, const void* const* data, const size_t* sizes,
                                             uint64_t max_image_size_pixels, hipdec_batch* recycle);
HIPDEC_API void hipdec_batch_free(hipdec_batch* b);
HIPDEC_API int hipdec_batch_count(const hipdec_batch* b);
HIPDEC_API int hipdec_batch_info(const hipdec_batch* b, int i, hipdec_image_info* info);
HIPDEC_API int hipdec_batch_run(hipdec_batch* b, void* stream);      /* asynchronous                 */
HIPDEC_API int hipdec_batch_status(hipdec_batch* b);                 /* waits for THIS batch's work (not the stream); device errors */
HIPDEC_API int hipdec_batch_read_plane(hipdec_batch* b, int i, int c, void* dst_host, size_t dst_stride);
HIPDEC_API int hipdec_batch_device_plane(hipdec_batch* b, int i, int c, const void** dptr, size_t* stride);
/* Grid / multi-GPU hand-over (device-side form of HeifPixelImage::copy_image_to,
 * libheif/image/pixelimage.cc:1115-1172): hipdec_batch_pack_item writes item i's cropped planes tightly
 * (Y then Cb then Cr, row stride = width * bytes per sample) into a caller-owned device buffer, e.g. the
 * send buffer of an RCCL gather; hipdec_copy2d_d2d pastes a plane into a canvas at the caller's offset.
 * Both are asynchronous on `stream`. */
HIPDEC_API size_t hipdec_batch_item_packed_bytes(const hipdec_batch* b, int i);
HIPDEC_API int hipdec_batch_pack_item(hipdec_batch* b, int i, void* dst_dev, size_t dst_bytes, void* stream);
HIPDEC_API int hipdec_copy2d_d2d(void* dst_dev, size_t dst_stride, const void* src_dev, size_t src_stride, size_t width_bytes,
                                 size_t height, void* stream);
/* Fused colour stage over item i (planes -> interleaved RGB in HBM), see hipdec_color_* below;
 * out_chroma uses heif_chroma numeric values (10 = RGB, 11 = RGBA, 12/14 = RRGGBB BE/LE). */
HIPDEC_API int hipdec_batch_to_rgb(hipdec_batch* b, int i, int out_chroma, void* out_dev, size_t out_stride,
                                   void* stream);
/* The same for ALL items of the batch as one kernel launch (outs_dev[i] / out_strides[i] per item; every item must
 * select the same output layout, which out_chroma guarantees). */
HIPDEC_API int hipdec_batch_to_rgb_all(hipdec_batch* b, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream);
/* hipdec_batch_run + hipdec_batch_to_rgb_all as one call.  For 8-bit 4:2:0 batches and interleaved RGB24 the colour conversion is FUSED into the
 * SAO kernel's store path (the planes are still written; the colour pass's re-read of them and its launch disappear); other cases run the two
 * steps one after the other.  Same pixels either way. */
HIPDEC_API int hipdec_batch_run_rgb(hipdec_batch* b, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream);
/* per-kernel device time of the last run in microseconds (HIP events on the launch stream):
 * [0] CABAC parse, [1] reconstruction, [2] deblock, [3] SAO + crop, [4] total */
HIPDEC_API int hipdec_batch_last_timing_us(hipdec_batch* b, float out[5]);
/* keep the events of the last `slots` runs (run k records into slot k % slots) so that a benchmark can
 * average per-kernel device time over its whole timed region without synchronising between runs */
HIPDEC_API int hipdec_batch_timing_slots(hipdec_batch* b, int slots);
HIPDEC_API int hipdec_batch_slot_timing_us(hipdec_batch* b, int slot, float out[5]);
/* the same per kernel: [0] CABAC parse, [1] residual (dequantisation + inverse transforms), [2] intra reconstruction,
 * [3] deblock, [4] SAO + crop, [5] colour stage (hipdec_batch_to_rgb_all after that run; 0 if none), [6] decode total
 * (parse .. SAO), [7] reserved */
HIPDEC_API int hipdec_batch_slot_kernel_timing_us(hipdec_batch* b, int slot, float out[8]);
/* debug / test taps of item i after a run (device -> host): which = 0 pre-deblock, 1 post-deblock */
HIPDEC_API int hipdec_batch_read_tap(hipdec_batch* b, int i, int which, int c, void* dst_host, size_t dst_stride);
HIPDEC_API int hipdec_batch_read_maps(hipdec_batch* b, int i, uint8_t* log2_tb, uint8_t* log2_cb, uint8_t* intra_luma,
                                      uint8_t* intra_chroma, int8_t* qp_y, uint8_t* flags, size_t map_elems);

/* ---- grid images across the GPUs of one node ------------------------------------------------- */
/* Device-side form of ImageItem_Grid::decode_full_grid_image + decode_and_paste_tile_image (libheif/image-items/grid.cc:250-468,
 * :482-577; HeifPixelImage::copy_image_to, libheif/image/pixelimage.cc:1115-1172) in ONE process over several HIP devices: tile
 * t = row * cols + col (order of the 'dimg' references) is decoded by shard t mod n_devices on that shard's device, each decoded
 * plane is pasted with one strided device-to-device copy (xGMI peer access where available) at its position in the canvas on
 * devices[0], clipped to the output size; the colour conversion then runs once over the canvas.
 * devices: n_devices device indices (entries may repeat: several shards on one device); NULL = devices 0 .. n_devices-1,
 * n_devices 0 = all visible devices.  tile_data[t] / tile_sizes[t]: the tiles in grid order, push_data framing. */
typedef struct hipdec_grid hipdec_grid;
HIPDEC_API int hipdec_grid_create(hipdec_grid** out, int rows, int cols, int out_width, int out_height, const void* const* tile_data,
                                  const size_t* tile_sizes, const int* devices, int n_devices, uint64_t max_image_size_pixels);
HIPDEC_API void hipdec_grid_free(hipdec_grid* g);
/* info of the composed image (width / height = output size, coded size = tiled area, VUI colour description of tile 0) */
HIPDEC_API int hipdec_grid_info(const hipdec_grid* g, hipdec_image_info* info, int* n_shards);
HIPDEC_API int hipdec_grid_decode(hipdec_grid* g);                  /* asynchronous: decode + paste queued on every shard */
HIPDEC_API int hipdec_grid_wait(hipdec_grid* g);                    /* waits for all shards; device-side errors */
HIPDEC_API int hipdec_grid_canvas_plane(hipdec_grid* g, int c, const void** dptr, size_t* stride, int* device);
HIPDEC_API int hipdec_grid_read_plane(hipdec_grid* g, int c, void* dst_host, size_t dst_stride);
/* hipdec_grid_read_plane, and the host copy is remembered as device-resident (the canvas stays alive behind it until the entry is used):
 * what the ImageItem_Grid fast path of libheif_amd/integration/image_ops_hip.cc fills the composed HeifPixelImage with, so that the colour
 * conversion that follows (hipdec_color_convert) reads the canvas on the device */
HIPDEC_API int hipdec_grid_read_plane_tracked(hipdec_grid* g, int c, void* dst_host, size_t dst_stride);
/* the planner + fused colour stage over the canvas (hipdec_color_convert); out on the host, or on devices[0] */
HIPDEC_API int hipdec_grid_to_rgb(hipdec_grid* g, int out_chroma, int upsampling, int only_preferred, void* out, size_t out_stride,
                                  int out_on_device);

/* shards on the root device / shards that write the canvas through enabled peer access (xGMI) / shards whose copies the runtime stages
 * (hipDeviceCanAccessPeer said no, or hipDeviceEnablePeerAccess failed) */
HIPDEC_API int hipdec_grid_transport(const hipdec_grid* g, int* local_shards, int* peer_shards, int* staged_shards);

/* ---- grid images, SPMD form: one process per GPU, tiles gathered with RCCL over xGMI ----------------------------
 * The same partition as hipdec_grid_* (tile t -> rank t mod nranks; libheif/image-items/grid.cc:405-453, :482-577) for hosts that run one
 * process per GPU: every rank decodes its tiles on its own device, one grouped ncclSend / ncclRecv gather brings the packed tiles
 * (Y | Cb | Cr, 1.5 B/px for 8-bit 4:2:0) to rank 0, which pastes them (HeifPixelImage::copy_image_to, image/pixelimage.cc:1115-1172) and runs
 * the colour conversion once over the canvas.  create / decode are COLLECTIVE: every rank of the communicator calls them, with the same grid
 * geometry.  `comm` is an ncclComm_t (the host's own, or one from hipdec_rccl_comm_create); librccl is loaded at run time - without it these
 * entry points return HIPDEC_ERR_UNSUPPORTED. */
#define HIPDEC_RCCL_UNIQUE_ID_BYTES 128
HIPDEC_API int hipdec_rccl_available(void);
HIPDEC_API int hipdec_rccl_unique_id(void* id_out /* HIPDEC_RCCL_UNIQUE_ID_BYTES, rank 0; the host sends it to the other ranks */);
HIPDEC_API int hipdec_rccl_comm_create(void** comm_out, int nranks, int rank, const void* unique_id);   /* ncclCommInitRank on the hipdec_init device */
HIPDEC_API void hipdec_rccl_comm_destroy(void* comm);
typedef struct hipdec_grid_rccl hipdec_grid_rccl;
/* tile_data[t] / tile_sizes[t]: needed for the tiles this rank owns (t mod nranks == rank); other entries may be NULL / 0 */
HIPDEC_API int hipdec_grid_create_rccl(hipdec_grid_rccl** out, void* comm, int rank, int nranks, int rows, int cols, int out_width, int out_height,
                                       const void* const* tile_data, const size_t* tile_sizes, uint64_t max_image_size_pixels);
HIPDEC_API void hipdec_grid_rccl_free(hipdec_grid_rccl* g);
HIPDEC_API int hipdec_grid_rccl_decode(hipdec_grid_rccl* g);   /* asynchronous: decode + gather + paste queued on the rank's stream */
HIPDEC_API int hipdec_grid_rccl_wait(hipdec_grid_rccl* g);     /* this rank's work, then ONE 8-byte all-reduce per decode: every rank - rank 0 with the canvas first of all -
                                                                  * learns whether every shard decoded.  EVERY rank must call it (or to_rgb / read_plane, which do) after each decode -
                                                                  * ALSO a rank whose decode() returned an error (its peers are inside the all-reduce); it then returns that error */
/* rank 0 only (it owns the canvas): */
HIPDEC_API int hipdec_grid_rccl_canvas_plane(hipdec_grid_rccl* g, int c, const void** dptr, size_t* stride);
HIPDEC_API int hipdec_grid_rccl_read_plane(hipdec_grid_rccl* g, int c, void* dst_host, size_t dst_stride);
HIPDEC_API int hipdec_grid_rccl_to_rgb(hipdec_grid_rccl* g, int out_chroma, int upsampling, int only_preferred, void* out, size_t out_stride,
                                       int out_on_device);

/* ---- colour stage ---------------------------------------------------------------------------- */
typedef struct hipdec_nclx {
  int has_nclx;               /* 0: the image carries no nclx profile (reference uses its defaults) */
  int colour_primaries, transfer_characteristics, matrix_coefficients, full_range_flag;
} hipdec_nclx;

/* Op_YCbCr420_to_RGB24 / Op_YCbCr420_to_RGB32 (libheif/color-conversion/yuv2rgb.cc:345-426,
 * :481-562): 8-bit 4:2:0, 8.8 fixed point, nearest-neighbour chroma, alpha filled with 0xFF. */
HIPDEC_API int hipdec_color_420_to_rgb24(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs,
                                         int w, int h, const hipdec_nclx* nclx, void* out, size_t out_stride,
                                         int with_alpha, void* stream);
/* Op_YCbCr_to_RGB<uint8_t/uint16_t> (yuv2rgb.cc:92-292): float32, NN chroma, planar R,G,B out with
 * the input's bit depth.  chroma: 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4. */
HIPDEC_API int hipdec_color_ycbcr_to_rgb_planar(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr,
                                                size_t crs, int w, int h, int bpp, int chroma, const hipdec_nclx* nclx,
                                                void* r, void* g, void* b, size_t out_stride, void* stream);
/* Op_YCbCr_to_RGB<uint8_t> followed by Op_RGB_to_RGB24_32 (rgb2rgb.cc:72-150) fused into one pass:
 * what libheif's planner runs for limited-range 8-bit input. */
HIPDEC_API int hipdec_color_ycbcr_to_rgb24_float(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr,
                                                 size_t crs, int w, int h, int chroma, const hipdec_nclx* nclx,
                                                 void* out, size_t out_stride, int with_alpha, void* stream);
/* Op_YCbCr420_to_RRGGBBaa (yuv2rgb.cc:622-734): >8-bit 4:2:0 -> 16-bit interleaved BE or LE. */
HIPDEC_API int hipdec_color_420_to_rrggbb(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs,
                                          int w, int h, int bpp, const hipdec_nclx* nclx, void* out, size_t out_stride,
                                          int little_endian, void* stream);
/* Op_YCbCr420_bilinear_to_YCbCr444<Pixel> (chroma_sampling.cc:501-724), one chroma plane;
 * (w, h) = luma size; reproduces the reference's border indexing. */
/* Op_mono_to_RGB24_32 (libheif/color-conversion/monochrome.cc): 8-bit monochrome plane -> RGB24 / RGBA32 (R = G = B = Y; alpha copied, or 0xFF) */
HIPDEC_API int hipdec_color_mono_to_rgb24(const void* y, size_t ys, const void* alpha, size_t alpha_stride, int w, int h, void* out,
                                          size_t out_stride, int with_alpha, void* stream);
/* > 8-bit planes (chroma 1 / 2 / 3) to 8-bit interleaved RGB(A) in one pass.  sdr_first = 1: Op_to_sdr_planes (hdr_sdr.cc:146-244) on the planes, then
 * Op_YCbCr420_to_RGB24 / _RGB32 (4:2:0 only); sdr_first = 0: Op_YCbCr_to_RGB<uint16_t>, Op_to_sdr_planes on R, G, B, Op_RGB_to_RGB24_32.  Which of
 * the two the reference's planner builds for a state: hipdec_color_plan. */
HIPDEC_API int hipdec_color_hdr_to_rgb24(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h,
                                         int bpp, int chroma, const hipdec_nclx* nclx, void* out, size_t out_stride, int with_alpha,
                                         int sdr_first, void* stream);
/* Op_YCbCr_to_RGB<uint16_t> (libheif/color-conversion/yuv2rgb.cc:92-292) + Op_RGB_HDR_to_RRGGBBaa_BE (rgb2rgb.cc:470-560) [+ the endianness swap]:
 * > 8-bit planes of any chroma format (1 / 2 / 3) to interleaved RRGGBB at the input bit depth, one pass */
HIPDEC_API int hipdec_color_ycbcr_to_rrggbb_float(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs,
                                                  int w, int h, int bpp, int chroma, const hipdec_nclx* nclx, void* out,
                                                  size_t out_stride, int little_endian, void* stream);
HIPDEC_API int hipdec_color_bilinear_420_to_444(const void* in, size_t is, int w, int h, int bpp, void* out, size_t os,
                                                void* stream);
/* Op_YCbCr422_bilinear_to_YCbCr444<Pixel> (chroma_sampling.cc:732-954), one chroma plane of ((w + 1) / 2) x h samples -> w x h. */
HIPDEC_API int hipdec_color_bilinear_422_to_444(const void* in, size_t is, int w, int h, int bpp, void* out, size_t os,
                                                void* stream);
/* Op_to_sdr_planes (hdr_sdr.cc:146-244): v >> (bits - 8), uint16 -> uint8. */
HIPDEC_API int hipdec_color_to_sdr(const void* in, size_t is, int w, int h, int bits, void* out, size_t os, void* stream);
/* Op_YCbCr420_to_RGB32 with a real alpha plane (yuv2rgb.cc:481-562; alpha copied as :552) when integer_op != 0, else the float
 * chain Op_YCbCr_to_RGB<uint8_t> + Op_RGB_to_RGB24_32 with the alpha plane interleaved (rgb2rgb.cc:72-150).  alpha NULL: 0xFF. */
HIPDEC_API int hipdec_color_420_to_rgba_alpha(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs,
                                              int w, int h, const hipdec_nclx* nclx, const void* alpha, size_t alpha_stride,
                                              int integer_op, int chroma, void* out, size_t out_stride, void* stream);

/* ---- the colour boundary: planner (a8) + image-level conversion ------------------------------------------------------
 * What ColorConversionPipeline::construct_pipeline + convert_image do for a decoded HEIC image
 * (libheif/color-conversion/colorconversion.cc:279-623), behind ONE call.  The integration op registered in init_ops()
 * (libheif_amd/integration/colorconversion_hip.cc) forwards to hipdec_color_convert(). */
typedef enum hipdec_color_op {   /* the reference operations a plan is made of */
  HIPDEC_OP_TO_SDR = 1,                 /* Op_to_sdr_planes                  hdr_sdr.cc:146-244 */
  HIPDEC_OP_BILINEAR_420_TO_444 = 2,    /* Op_YCbCr420_bilinear_to_YCbCr444  chroma_sampling.cc:501-724 */
  HIPDEC_OP_420_TO_RGB24 = 3,           /* Op_YCbCr420_to_RGB24              yuv2rgb.cc:345-426 */
  HIPDEC_OP_420_TO_RGB32 = 4,           /* Op_YCbCr420_to_RGB32              yuv2rgb.cc:481-562 */
  HIPDEC_OP_YCBCR_TO_RGB = 5,           /* Op_YCbCr_to_RGB<Pixel>            yuv2rgb.cc:92-292 */
  HIPDEC_OP_RGB_TO_RGB24_32 = 6,        /* Op_RGB_to_RGB24_32                rgb2rgb.cc:72-150 (fused into the op before it) */
  HIPDEC_OP_420_TO_RRGGBB = 7,          /* Op_YCbCr420_to_RRGGBBaa           yuv2rgb.cc:622-734 */
  HIPDEC_OP_BILINEAR_422_TO_444 = 8,    /* Op_YCbCr422_bilinear_to_YCbCr444  chroma_sampling.cc:732-954 */
  HIPDEC_OP_RGB_HDR_TO_RRGGBB_BE = 9,   /* Op_RGB_HDR_to_RRGGBBaa_BE         rgb2rgb.cc (fused into the op before it) */
  HIPDEC_OP_SWAP_ENDIANNESS = 10,       /* Op_RRGGBBaa_swap_endianness       rgb2rgb.cc:647-764 (fused likewise) */
  HIPDEC_OP_MONO_TO_RGB24_32 = 11       /* Op_mono_to_RGB24_32               monochrome.cc (input chroma 0 = heif_chroma_monochrome) */
} hipdec_color_op;

typedef struct hipdec_color_image {
  int width, height;       /* luma size */
  int chroma;              /* heif_chroma of the planes: 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4 */
  int bit_depth;
  const void* plane[4];    /* Y, Cb, Cr, alpha (NULL: none) */
  size_t stride[4];        /* bytes */
  int on_device;           /* 0: host pointers (libheif's HeifPixelImage planes), 1: device pointers */
} hipdec_color_image;

/* a8: the chain the reference's planner selects for (input state, output heif_chroma, chroma-upsampling options:
 * upsampling 1 = nearest neighbour, 2 = bilinear; only_preferred as heif_color_conversion_options).  HIPDEC_ERR_UNSUPPORTED for
 * states outside the HEIC hot path (the stock ops keep those). */
HIPDEC_API int hipdec_color_plan(int bit_depth, int chroma, int has_alpha, const hipdec_nclx* nclx, int out_chroma, int upsampling,
                                 int only_preferred, int ops[8], int* n_ops);
/* plan + execute on the GPU.  Host planes that a hipdec decoder has just handed to libheif (hipdec_decoder_read_plane_tracked)
 * are read from their device-resident copy, others are uploaded; `out` is a host buffer (or a device buffer, out_on_device). */
HIPDEC_API int hipdec_color_convert(const hipdec_color_image* in, const hipdec_nclx* nclx, int out_chroma, int upsampling,
                                    int only_preferred, void* out, size_t out_stride, int out_on_device);
/* ---- transformative item properties on the device: what ImageItem::decode_image applies to the decoded image on the host
 * (libheif/image-items/image_item.cc:949-1081: 'irot' :958-966, 'imir' :968-977, 'clap' :981-1010) ---------------------------------------- */
typedef enum hipdec_transform_op {
  HIPDEC_XF_ROTATE_CCW = 0,   /* args[0] = 90 / 180 / 270      HeifPixelImage::rotate_ccw      libheif/image/pixelimage.cc:1175-1333 */
  HIPDEC_XF_MIRROR = 1,       /* args[0] = heif_transform_mirror_direction (0 vertical, 1 horizontal)   mirror_inplace   :1337-1430 */
  HIPDEC_XF_CROP = 2          /* args = left, right, top, bottom (inclusive end points)        HeifPixelImage::crop            :1433-1530 */
} hipdec_transform_op;
/* Every plane of `in` (host or device pointers; host planes the decoder handed over are found device-resident) through the op, into the planes
 * `out` brings (same on_device convention; NULL where `in` has no plane); out->width / height / chroma / bit_depth are filled in.  Returns
 * HIPDEC_ERR_UNSUPPORTED where the reference converts the image to 4:4:4 first (odd size / offset of a subsampled image) and for odd crop
 * windows of subsampled images (half-covered chroma edge): the caller keeps the host path there. */
HIPDEC_API int hipdec_image_transform(const hipdec_color_image* in, int op, const int* args, hipdec_color_image* out);
/* the plane kernels (device pointers, `stream` a hipStream_t or NULL): ComponentStorage::rotate_ccw<T> / mirror_inplace<T> (pixelimage.cc:1305-1355)
 * and the per-plane copy of HeifPixelImage::crop; bytes_per_sample 1 or 2 */
HIPDEC_API int hipdec_plane_rotate_ccw(const void* in, size_t in_stride, int w, int h, int bytes_per_sample, int angle, void* out, size_t out_stride, void* stream);
HIPDEC_API int hipdec_plane_mirror(const void* in, size_t in_stride, int w, int h, int bytes_per_sample, int direction, void* out, size_t out_stride, void* stream);
HIPDEC_API int hipdec_plane_crop(const void* in, size_t in_stride, int w, int h, int bytes_per_sample, int left, int top, int out_w, int out_h, void* out,
                                 size_t out_stride, void* stream);

/* ---- scaled output (thumbnails) on the device -------------------------------------------------------------------------------------------------
 * What applications do with heif_image_scale_image() right after heif_decode_image() (libheif/api/libheif/heif_image.cc:240; examples/heif_thumbnailer.cc:197),
 * without the full-size picture leaving HBM.  Two filters:
 *  HIPDEC_SCALE_NEAREST  HeifPixelImage::scale_nearest_neighbor (libheif/image/pixelimage.cc:1783-1972) bit for bit: output sample (x, y) of EVERY plane is
 *                        input sample (x * in_width / out_width, y * in_height / out_height) of that plane (64-bit products), with the IMAGE's sizes also for
 *                        the chroma planes; the output chroma planes have the subsampled size of the output image ((w + 1) / 2 ...).  Up-scaling is allowed.
 *  HIPDEC_SCALE_BOX      area average (not in the reference), integer-exact.  A plane of pw x ph samples goes to qw x qh: output sample (ox, oy) is
 *                        (S + n / 2) / n, S the sum of the input samples in [x0, x1) x [y0, y1), x0 = ox * pw / qw, x1 = (ox + 1) * pw / qw (x0 + 1 where that
 *                        left the range empty), the same in y, n = (x1 - x0) * (y1 - y0); 64-bit products, integer division.  Each plane uses ITS OWN pw, ph.
 * Two more filters are taken by the tensor forms and the interleaved RGB24 forms further down, NOT by the plane-level calls of this section
 * (hipdec_image_scale, hipdec_plane_scale, hipdec_batch_read_plane_scaled keep refusing them as unknown filters):
 *  HIPDEC_SCALE_BILINEAR, HIPDEC_SCALE_BICUBIC   Pillow's 8-bit resampler (PIL.Image.resize with BILINEAR / BICUBIC; src/libImaging/Resample.c), bit for bit.
 *  For an entry with window rw x rh at (left, top) and pre-orientation output ow x oh:
 *      V = resample(full[top : top + rh, left : left + rw], ow, oh),
 *  `full` the interleaved 8-bit RGB picture hipdec_batch_to_rgb writes for out_chroma 10 (nearest-neighbour chroma, the planner's op, to-SDR for sources above
 *  8 bits) - that is Image.fromarray(full).crop(window).resize((ow, oh), filter).  The window is the image: nothing outside it is read.  The flip, the float
 *  stage and the orientation apply to V exactly as they do for the other filters.  resample is separable, the horizontal pass first, the intermediate rounded
 *  and clipped to 8 bits between the passes.  Per axis, n_in input and n_out output samples, all in IEEE double without contraction:
 *      scale = (double)n_in / n_out;  fs = max(scale, 1.0);  support = S * fs   (S = 1.0 bilinear, 2.0 bicubic);  ss = 1.0 / fs
 *      for xx in [0, n_out):  center = (xx + 0.5) * scale
 *          xmin = max((int)(center - support + 0.5), 0);   xmax = min((int)(center + support + 0.5), n_in);   n = xmax - xmin
 *          w[x] = f((x + xmin - center + 0.5) * ss), x in [0, n);   ww = w[0] + w[1] + ... in that order;   if (ww != 0.0) w[x] /= ww
 *          k[x] = (int)(w[x] * 4194304.0 + (w[x] < 0 ? -0.5 : 0.5))                 (2^22; the conversion truncates toward zero)
 *          out[xx] = clip((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)         (int32 accumulation, arithmetic shift)
 *      bilinear  f(x): x = |x|;  x < 1 ? 1.0 - x : 0.0
 *      bicubic   f(x): x = |x|, a = -0.5;  x < 1: ((a + 2.0) * x - (a + 3.0)) * x * x + 1;   x < 2: (((x - 5) * x + 8) * x - 4) * a;   else 0.0
 *  (Pillow skips a pass whose axis keeps its size; both filters give the identity kernel there.)  A monochrome source gives R = G = B.  Sources above 8 bits
 *  are taken with HIPDEC_TENSOR_U8 and by the RGB24 forms; a float dtype from such a source would need a native-depth definition Pillow does not have and is
 *  HIPDEC_ERR_UNSUPPORTED.  The RGB forms take these filters for out_chroma 10 only (any other: HIPDEC_ERR_UNSUPPORTED).  The coefficient tables are computed
 *  on the host, one per distinct (n_in, n_out) of a call, and uploaded with one copy; a call whose tables exceed 64 MiB is HIPDEC_ERR_LIMIT before anything
 *  is launched (a table holds about 2 * S * n_in + 3 * n_out 32-bit values: a 4096-sample axis to 224 with bicubic is 66 KB). */
typedef enum hipdec_scale_filter { HIPDEC_SCALE_NEAREST = 0, HIPDEC_SCALE_BOX = 1, HIPDEC_SCALE_BILINEAR = 16, HIPDEC_SCALE_BICUBIC = 17 } hipdec_scale_filter;
/* Host only (no device is touched): the taps of output sample out_index along an axis of in_size -> out_size samples as the kernel receives them.  Returns their
 * count n (< 0: error), *first = xmin, coeffs[0 .. min(n, capacity)) = k[].  filter: HIPDEC_SCALE_BILINEAR or HIPDEC_SCALE_BICUBIC. */
HIPDEC_API int hipdec_resample_taps(int in_size, int out_size, int filter, int out_index, int* first, int32_t* coeffs, int capacity);
/* Every plane of `in` (host or device pointers as `on_device` says; host planes the decoder handed over are found device-resident) to out_width x out_height,
 * into the planes `out` brings (same on_device convention; NULL where `in` has none); out->width / height / chroma / bit_depth are filled in.  The chroma
 * format is kept: chroma planes come out at the subsampled size of the output image. */
HIPDEC_API int hipdec_image_scale(const hipdec_color_image* in, int out_width, int out_height, int filter, hipdec_color_image* out);
/* counter since load: images through hipdec_image_scale */
HIPDEC_API void hipdec_image_scale_stats(uint64_t* images);
/* the plane kernel (device pointers; synchronises `stream`): a plane of in_w x in_h samples to out_w x out_h.  image_w / image_h -> image_out_w / image_out_h
 * are the sizes of the IMAGE the plane belongs to, which the nearest-neighbour index uses (for a luma or a lone plane: the plane's own); the box filter
 * only looks at the plane's sizes.  bytes_per_sample 1 or 2. */
HIPDEC_API int hipdec_plane_scale(const void* in, size_t in_stride, int in_w, int in_h, int bytes_per_sample, int image_w, int image_h, int image_out_w,
                                  int image_out_h, int out_w, int out_h, int filter, void* out, size_t out_stride, void* stream);
/* hipdec_batch_to_rgb with a scaled result: interleaved rows of out_width x out_height pixels straight from item i's decoded planes, ONE fused kernel (no
 * full-size RGB and no scaled planes in HBM).  Every out_chroma / bit depth / chroma format hipdec_batch_to_rgb takes, monochrome included.
 *  nearest: the bytes of hipdec_batch_to_rgb at full size followed by the reference's interleaved scaling (pixelimage.cc:1876-1886):
 *           out(x, y) = full(x * W / out_width, y * H / out_height); only the sampled pixels are read.
 *  box:     the bytes of hipdec_color_convert (nearest-neighbour upsampling has nothing to do) on the three planes box-scaled to out_width x out_height each,
 *           i.e. on a 4:4:4 image of the input's bit depth and VUI colour description.
 *  bilinear / bicubic (out_chroma 10 only): resample(full, out_width, out_height) as defined above, `full` the bytes of hipdec_batch_to_rgb.
 * HIPDEC_ERR_LIMIT when the batch was created with max_image_size_pixels and out_width x out_height exceeds it.  Asynchronous on `stream`. */
HIPDEC_API int hipdec_batch_to_rgb_scaled(hipdec_batch* b, int i, int out_chroma, int out_width, int out_height, int filter, void* out_dev, size_t out_stride,
                                          void* stream);
/* the same for ALL items as one launch, with per-item sizes (out_widths[i] x out_heights[i] into outs_dev[i] / out_strides[i]); the device time lands in
 * slot [5] of hipdec_batch_slot_kernel_timing_us like hipdec_batch_to_rgb_all's */
HIPDEC_API int hipdec_batch_to_rgb_scaled_all(hipdec_batch* b, int out_chroma, const int* out_widths, const int* out_heights, int filter, void* const* outs_dev,
                                              const size_t* out_strides, void* stream);
/* plane c of item i as hipdec_image_scale would hand it out for an image of out_width x out_height (c > 0: the subsampled size of that), into a host buffer */
HIPDEC_API int hipdec_batch_read_plane_scaled(hipdec_batch* b, int i, int c, int out_width, int out_height, int filter, void* dst_host, size_t dst_stride);

/* ---- tensor output on the device: cropped, scaled, normalised batches ---------------------------------------------------------------------------
 * What a training-data loader builds from decoded pictures: a crop window per sample, an optional horizontal flip, one common output size, float values
 * already multiplied and shifted, one dense tensor.  ONE fused kernel from the decoded planes: no full-size RGB, no scaled intermediate in HBM.
 *
 * Output: n_entries samples of three channels R, G, B (a monochrome source gives R = G = B).  Entry e starts at element e * 3 * height * width; NCHW places
 * element (c, y, x) at (c * height + y) * width + x, NHWC at (y * width + x) * 3 + c; there is no padding.
 * Entries: `item` selects the batch item (the image form ignores it); [left, left + width) x [top, top + height) is a window in luma samples of the
 * cropped picture, at any offset and parity; all zeros after `item` mean the whole picture; flip != 0 mirrors the result horizontally (output column x
 * holds what column width - 1 - x would hold).  Several entries may name one item; up-scaling is allowed.
 * Integer stage, rw x rh the window and ow x oh the output:
 *  HIPDEC_SCALE_NEAREST  V(x, y) = full(left + x * rw / ow, top + y * rh / oh), `full` the picture hipdec_batch_to_rgb writes (64-bit products, integer
 *                        division).  For the whole picture: hipdec_batch_to_rgb_scaled NEAREST.
 *  HIPDEC_SCALE_BOX      the box definition above applied to each plane CROPPED to the window, with that plane's own cropped size: luma columns
 *                        [left, left + rw), chroma columns [left >> sH, ((left + rw - 1) >> sH) + 1), the same in y with sV; then the colour conversion
 *                        of hipdec_color_convert on the three averaged planes as a 4:4:4 image.  For the whole picture: hipdec_batch_to_rgb_scaled BOX.
 *  HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC   V = resample(full[window], ow, oh), Pillow's resampler as defined with hipdec_scale_filter; 8-bit component
 *                        values only (a float dtype from a source above 8 bits: HIPDEC_ERR_UNSUPPORTED).
 *  The component value V is the out_chroma 10 value (8 bits; sources above 8 bits go through to-SDR) for 8-bit sources and for HIPDEC_TENSOR_U8 from any
 *  source; float dtypes from sources above 8 bits get the native-depth value out_chroma 14 would store (0 .. 2^bits - 1: fold 1 / 1023 into `scale`).
 * Float stage: (float)V * scale[c] + bias[c] in fp32 - a multiply, then an add, each rounded once - and for F16 / BF16 the IEEE round-to-nearest-even
 * conversion of that value, subnormals included.  HIPDEC_TENSOR_U8 stores V and ignores scale / bias. */
typedef enum hipdec_tensor_dtype { HIPDEC_TENSOR_U8 = 0, HIPDEC_TENSOR_F32 = 1, HIPDEC_TENSOR_F16 = 2, HIPDEC_TENSOR_BF16 = 3 } hipdec_tensor_dtype;
typedef enum hipdec_tensor_layout { HIPDEC_TENSOR_NCHW = 0, HIPDEC_TENSOR_NHWC = 1 } hipdec_tensor_layout;
typedef struct hipdec_tensor_desc {
  int width, height;       /* of every sample */
  int dtype, layout;       /* hipdec_tensor_dtype, hipdec_tensor_layout */
  int filter;              /* hipdec_scale_filter */
  int reserved;            /* 0 */
  float scale[3], bias[3]; /* per channel R, G, B */
} hipdec_tensor_desc;
typedef struct hipdec_tensor_entry { int item, left, top, width, height, flip; } hipdec_tensor_entry;
/* bytes of a tensor of n_entries samples (0 for a description that would be refused) */
HIPDEC_API size_t hipdec_tensor_bytes(const hipdec_tensor_desc* desc, int n_entries);
/* All entries as ONE launch (65535 entries per launch), asynchronous on `stream`; the device time lands in slot [5] of hipdec_batch_slot_kernel_timing_us.
 * entries NULL: n_entries must be the item count, entry i = the whole of item i.  A window that leaves the picture, a non-positive size, an unknown dtype,
 * layout or filter, non-finite scale / bias with a float dtype, out_bytes below hipdec_tensor_bytes: HIPDEC_ERR_INVALID_ARGUMENT; width * height above the
 * batch's max_image_size_pixels: HIPDEC_ERR_LIMIT.  Sources of all entries are 8-bit, or all wider. */
HIPDEC_API int hipdec_batch_to_tensor(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, int n_entries, void* out_dev,
                                      size_t out_bytes, void* stream);
/* The single-image form over any hipdec_color_image (host or device planes; host planes the decoder handed over are found device-resident), with the planner
 * rules of hipdec_color_convert (nclx, range, matrix; nearest-neighbour chroma).  plane[3] is ignored; entries NULL: n_entries must be 1, the whole image.
 * `out` is a host buffer, or a device buffer with out_on_device.  Synchronises. */
HIPDEC_API int hipdec_image_to_tensor(const hipdec_color_image* in, const hipdec_nclx* nclx, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries,
                                      int n_entries, void* out, size_t out_bytes, int out_on_device);
/* counters since load: tensors written by the two calls above, and their entries */
HIPDEC_API void hipdec_tensor_stats(uint64_t* tensors, uint64_t* entries);
/* Debug inspection: plane `plane` (0 .. 2) of entry `entry` as the kernel of the batch's LAST hipdec_batch_to_tensor received it - the device pointer and
 * stride of the PLANE and the window of it that is scaled.  A window is carried as an offset and never moves the pointer, so the box kernel's aligned
 * 32- / 64-bit row loads start at a 4-sample boundary of the plane whatever the window's parity.  (Calls with the bilinear / bicubic filters keep their blocks
 * apart and are not what this call shows.) */
HIPDEC_API int hipdec_batch_tensor_block(hipdec_batch* b, int entry, int plane, const void** plane_dev, size_t* plane_stride, int* x, int* y, int* width,
                                         int* height);

/* ---- albums of grid photos: K photos, ONE launch set, ONE fused paste ---------------------------------------------------------------------------------
 * hipdec_grid_* composes one photo per object, so a host with an album pays one launch set per photo, each bound by a single tile's CABAC critical path.
 * An album takes the tiles of all its photos into ONE hipdec_batch (the album owns it), so their substreams fill the CABAC pool together, and pastes
 * every tile plane of every photo into its canvas - HeifPixelImage::copy_image_to (libheif/image/pixelimage.cc:1115-1172), clipped to the photo's output
 * size - with ONE kernel launch over a job table.  The canvases stay in HBM until hipdec_album_free and feed the colour, scaled and tensor stages of the
 * batch forms, one launch each.
 *  photos[p]: a grid of rows x cols tiles (1 .. 256 each way) with output out_width x out_height; its tiles are tile_data[first_tile .. first_tile +
 *  rows * cols - 1] in 'dimg' order (push_data framing).  Tile ranges lie inside n_tiles and do not overlap; reserved is 0.  Photos may differ in grid
 *  geometry, tile size and output size; the album has one chroma format and one bit depth.  Per photo the rules of hipdec_grid_create hold: tiles of
 *  one size, the output fits the tiled area, no subsampled tiles with odd dimensions.  max_image_size_pixels bounds every tile and every photo's output.
 *  Whatever the arguments alone decide is refused before the library touches a device; what the tiles' headers decide, before anything is allocated.
 * Out of scope: sharding an album over several devices (hipdec_grid_* remains the multi-GPU form), alpha and auxiliary images, the libheif integration
 * hook, decoding straight into the canvas. */
typedef struct hipdec_album hipdec_album;
typedef struct hipdec_album_photo { int rows, cols, out_width, out_height, first_tile, reserved; } hipdec_album_photo;
HIPDEC_API int hipdec_album_create(hipdec_album** out, int n_photos, const hipdec_album_photo* photos, const void* const* tile_data,
                                   const size_t* tile_sizes, int n_tiles, uint64_t max_image_size_pixels);
HIPDEC_API void hipdec_album_free(hipdec_album* a);
HIPDEC_API int hipdec_album_count(const hipdec_album* a);           /* photos (a NULL album is an error, as for every call here) */
/* info of the composed photo, as hipdec_grid_info (output size, coded size = tiled area, VUI colour description of the photo's tile 0) */
HIPDEC_API int hipdec_album_info(const hipdec_album* a, int photo, hipdec_image_info* info);
/* asynchronous: the batch's launch set over all tiles, then ONE paste launch (more than 65535 tile planes take as few launches as the grid size allows) */
HIPDEC_API int hipdec_album_run(hipdec_album* a, void* stream);
HIPDEC_API int hipdec_album_status(hipdec_album* a);                /* as hipdec_batch_status: waits for the album's work; device errors */
/* plane c of photo's canvas in HBM (rows of the output size, 256-byte-aligned stride; the bytes between a row's end and its stride are unspecified) */
HIPDEC_API int hipdec_album_canvas_plane(hipdec_album* a, int photo, int c, const void** dptr, size_t* stride);
HIPDEC_API int hipdec_album_read_plane(hipdec_album* a, int photo, int c, void* dst_host, size_t dst_stride);
/* hipdec_batch_to_rgb_all / _to_rgb_scaled_all / _to_tensor over pictures whose planes are the canvases: the same colour entry points, planner rules
 * (nearest-neighbour chroma), refusals and window rules, one launch per call; outs_dev[p] / out_widths[p] / entry.item name photo p. */
HIPDEC_API int hipdec_album_to_rgb_all(hipdec_album* a, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream);
HIPDEC_API int hipdec_album_to_rgb_scaled_all(hipdec_album* a, int out_chroma, const int* out_widths, const int* out_heights, int filter,
                                              void* const* outs_dev, const size_t* out_strides, void* stream);
HIPDEC_API int hipdec_album_to_tensor(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, int n_entries,
                                      void* out_dev, size_t out_bytes, void* stream);
/* counters since load: albums created, their photos, paste launches (exactly one per hipdec_album_run) */
HIPDEC_API void hipdec_album_stats(uint64_t* albums, uint64_t* photos, uint64_t* paste_launches);
/* measurement aid: device time of the paste of the last hipdec_album_run in microseconds (HIP events around its launch); waits for it */
HIPDEC_API int hipdec_album_paste_timing_us(hipdec_album* a, float* us);

/* ---- oriented output: 'irot' / 'imir' folded into the scaled RGB and tensor kernels ----------------------------------------------------------------------
 * Every phone HEIC carries an orientation.  hipdec_image_transform applies it plane by plane at full size before the colour stage; these calls apply it in
 * the store of the ONE fused launch that scales, converts and normalises, so a portrait thumbnail or training sample costs no second pass.
 *
 * hipdec_orientation: code = r + 4 * m.  The displayed picture is the stored picture rotated COUNTER-CLOCKWISE by r quarter turns, then mirrored
 * horizontally if m is set.  A quarter turn is HeifPixelImage::rotate_ccw(90): out(X, Y) = in(x = w - 1 - Y, y = X), the output is h x w; the horizontal
 * mirror is out(X, Y) = in(W - 1 - X, Y).  (NumPy, on an (H, W, ...) array: np.rot90(a, r), then np.fliplr if m.)
 * The host folds an item's 'ipma'-ordered 'irot' / 'imir' list into one code with hipdec_orientation_compose; reading the properties is the caller's. */
typedef enum hipdec_orientation {
  HIPDEC_ORIENT_0 = 0, HIPDEC_ORIENT_CCW90 = 1, HIPDEC_ORIENT_180 = 2, HIPDEC_ORIENT_CCW270 = 3,
  HIPDEC_ORIENT_MIRROR = 4, HIPDEC_ORIENT_CCW90_MIRROR = 5, HIPDEC_ORIENT_180_MIRROR = 6, HIPDEC_ORIENT_CCW270_MIRROR = 7
} hipdec_orientation;
/* Host only (no device is touched).  The code of "apply `op` to the displayed picture of `orientation`": op HIPDEC_XF_ROTATE_CCW with arg 90 / 180 / 270,
 * or HIPDEC_XF_MIRROR with arg 0 (vertical) / 1 (horizontal).  Anything else: -1, and hipdec_last_error says why. */
HIPDEC_API int hipdec_orientation_compose(int orientation, int op, int arg);
/* Host only.  The code of EXIF orientation 1 .. 8; anything else: -1. */
HIPDEC_API int hipdec_orientation_from_exif(int exif);
/* THE DEFINITION OF THE RESULT.  Output sizes are sizes of the DISPLAYED picture (desc->width x height, out_widths[i] x out_heights[i]), ow x oh below.
 *  - For an even r, the pre-orientation result P is what the unoriented call (hipdec_batch_to_tensor, hipdec_batch_to_rgb_scaled_all, and the album forms)
 *    writes for the same item, window, filter and size ow x oh; for an odd r, what it writes for size oh x ow (width oh, height ow).
 *  - The oriented result is orient(code, P), applied to PIXELS.  The integer stage, the float stage and the to-SDR rules are untouched.
 *  - Tensor entry windows stay in luma samples of the STORED picture, exactly as in the unoriented call.
 *  - An entry's flip mirrors the displayed result: fliplr^flip(orient(code, P)) (= the code hipdec_orientation_compose(code, HIPDEC_XF_MIRROR, 1)).
 * This agrees with libheif's own order - transform the planes, then convert with nearest-neighbour chroma - for 4:4:4 and 4:0:0 pictures, and for subsampled
 * pictures of even size.  For odd sizes of subsampled pictures the reference converts to 4:4:4 before it transforms; there the definition above is what holds.
 *
 * Tensor forms: as hipdec_batch_to_tensor / hipdec_album_to_tensor, with orientations[e] the code of entry e (NULL: all 0).
 * RGB forms: out_chroma 10 (interleaved RGB24) only, from 8-bit or wider sources (wider ones through to-SDR, as in the scaled call); any other out_chroma is
 * HIPDEC_ERR_UNSUPPORTED.  orientations[i] is the code of item / photo i (NULL: all 0); rows of picture i are out_strides[i] bytes apart and the bytes between
 * a row's end and the stride are not written.  Full-size oriented RGB is HIPDEC_SCALE_NEAREST at the displayed full size (the identity index map).
 * Everything the unoriented call refuses is refused with the same status; a code outside 0 .. 7 is HIPDEC_ERR_INVALID_ARGUMENT and names the entry; an
 * out_stride below 3 * out_width is refused; whatever the arguments alone decide is refused before a device is touched.  ONE launch per call (65535 entries per
 * launch), entries of different orientation share it; the device time lands in slot [5] of hipdec_batch_slot_kernel_timing_us like the sibling calls'. */
HIPDEC_API int hipdec_batch_to_tensor_oriented(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                               int n_entries, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_oriented(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                               int n_entries, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_rgb_scaled_oriented_all(hipdec_batch* b, int out_chroma, const int* orientations, const int* out_widths, const int* out_heights,
                                                       int filter, void* const* outs_dev, const size_t* out_strides, void* stream);
HIPDEC_API int hipdec_album_to_rgb_scaled_oriented_all(hipdec_album* a, int out_chroma, const int* orientations, const int* out_widths, const int* out_heights,
                                                       int filter, void* const* outs_dev, const size_t* out_strides, void* stream);
/* counters since load: launches of the oriented kernels, the entries they wrote, and how many of those had a quarter turn (odd r) */
HIPDEC_API void hipdec_oriented_stats(uint64_t* launches, uint64_t* entries, uint64_t* quarter_turn_entries);

/* ---- placed tensor output: letterbox and pad-to-size in the fused kernels ---------------------------------------------------------------------------------
 * The tensor forms above stretch every window to the one common desc->width x height.  Detection, segmentation, OCR and vision-language loaders keep the
 * aspect ratio (letterbox to 640 x 640 with grey 114) or pad to a common size (nested tensors with a padding mask, pad-to-max of a bucket).  These calls
 * write each sample into a rectangle of a larger canvas and fill the rest, in the same launch set: no scaled intermediate, no canvas fill, no copies.
 *
 * THE DEFINITION OF THE RESULT.  desc->width x height is the size of the CANVAS of every entry; layout, dtypes and hipdec_tensor_bytes are unchanged.
 * For entry e with rectangle pl = places[e] (the rectangle of the DISPLAYED sample inside the canvas):
 *  - Inside the rectangle the canvas holds, element for element, what hipdec_batch_to_tensor_oriented writes for the same entry (item, window, flip),
 *    orientation code, filter, dtype, scale and bias with desc->width / height replaced by pl.width / pl.height: canvas element (c, pl.y + Y, pl.x + X) is
 *    element (c, Y, X) of that result.  The pre-orientation size is swapped for an odd number of quarter turns exactly as that call defines it; the flip
 *    mirrors the sample inside its rectangle, not the canvas.  All filters, codes, dtypes and both layouts are taken; whatever the oriented call refuses
 *    for a sample of pl.width x pl.height is refused here with the same status.
 *  - Everywhere else the canvas holds the fill element of its channel:
 *      HIPDEC_FILL_COMPONENT  value[c] is an integral component value V in the range a pixel can have (0 .. 255; 0 .. 2^bits - 1 for a float dtype from a
 *                             source above 8 bits).  The element is what a pixel of that value gets: (float)V * scale[c] + bias[c], narrowed as pixels
 *                             are; V itself for HIPDEC_TENSOR_U8.  "Pad with 114, then normalise" is bit-identical to normalising a padded picture.
 *      HIPDEC_FILL_ELEMENT    value[c] is the element itself: stored as fp32, or narrowed to F16 / BF16 with the round-to-nearest-even statement of the
 *                             pixels (subnormals included); for HIPDEC_TENSOR_U8 an integer in 0 .. 255.  Zero-after-normalisation padding.
 *    fill NULL: component 0 in every channel.
 *  - mask_dev (may be NULL): a dense n_entries x height x width uint8 tensor, 1 where the canvas element is margin, 0 inside the rectangle.  Every byte of
 *    it is written.
 * places NULL: every rectangle is the whole canvas; with mask_dev NULL as well the call IS hipdec_batch_to_tensor_oriented, byte for byte and launch for
 * launch.  orientations NULL: all 0.  entries NULL: as in the sibling calls.
 * Refused before a device is touched, HIPDEC_ERR_INVALID_ARGUMENT: a rectangle with a non-positive side or one that leaves the canvas (the entry is named),
 * a non-finite fill, a component fill that is not integral or out of range, an unknown domain, a non-zero `reserved`, a U8 element fill that is not an
 * integer in 0 .. 255, out_bytes below hipdec_tensor_bytes, a code outside 0 .. 7.  Canvas width * height above max_image_size_pixels: HIPDEC_ERR_LIMIT.
 * (A component fill above 255 with a float dtype is held against the bit depth of the entries' sources: refused before anything is launched.)
 * Launches: the picture part through the oriented / resampling kernels with the canvas row as pitch and the canvas plane as plane stride; the margins of ALL
 * entries - and the mask - in ONE launch of k_canvas_margin (65535 entries per launch).  The two write disjoint elements, every canvas element exactly once.
 * A call without margins and without a mask launches no margin kernel.  Device time: slot [5] of hipdec_batch_slot_kernel_timing_us, both launches. */
typedef struct hipdec_tensor_place { int x, y, width, height; } hipdec_tensor_place;
typedef enum hipdec_fill_domain { HIPDEC_FILL_COMPONENT = 0, HIPDEC_FILL_ELEMENT = 1 } hipdec_fill_domain;
typedef struct hipdec_tensor_fill { float value[3]; int domain; int reserved; } hipdec_tensor_fill;
HIPDEC_API int hipdec_batch_to_tensor_placed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_placed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
/* Host only, 64-bit integer arithmetic.  The rectangle of a displayed sample of src_width x src_height fitted into the canvas with its aspect ratio kept:
 * with !upscale a source that fits both ways keeps its size; otherwise, if src_width * canvas_height >= src_height * canvas_width, width = canvas_width and
 * height = max(1, (src_height * canvas_width + src_width / 2) / src_width), else the mirror-image rule with height = canvas_height.  anchor 0: top-left;
 * 1: centred, x = (canvas_width - width) / 2 rounding down, the same for y.  A non-positive size or an unknown anchor: -1, hipdec_last_error says why. */
HIPDEC_API int hipdec_letterbox_place(int src_width, int src_height, int canvas_width, int canvas_height, int upscale, int anchor, hipdec_tensor_place* out);
/* counters since load: placed calls, their entries, launches of the margin kernel */
HIPDEC_API void hipdec_placed_stats(uint64_t* calls, uint64_t* entries, uint64_t* margin_launches);

/* ---- framed tensor output: resize-then-crop and crop-with-padding in one launch ------------------------------------------------------------------------
 * Resize(256) -> CenterCrop(224) (the evaluation pipeline of ImageNet models, CLIP / SigLIP preprocessing), RandomCrop(size, padding, pad_if_needed) and
 * detection-style jitter all RESIZE the picture and then cut a canvas out of it - or out of it and the padding around it.  An entry's window is a crop of
 * the stored picture taken BEFORE the resize, which is another operation: the crop rectangle of a resized picture maps back to a non-integer window, and
 * Pillow clamps the filter support at the edge of what it resizes, so border pixels differ.  The placed calls refuse a rectangle that leaves the canvas.
 * These calls take it: the rectangle of the resized sample may leave the canvas on any side, and only its visible part is computed and written.
 *
 * THE DEFINITION OF THE RESULT.  desc->width x height is the CANVAS of every entry - the crop size.  pl = places[e] is the rectangle of the resized,
 * DISPLAYED sample in canvas coordinates: pl.x and pl.y may be negative, pl.x + pl.width and pl.y + pl.height may exceed the canvas.  The VISIBLE PART is
 * the intersection of pl with the canvas.
 *  - Inside the visible part, canvas element (c, pl.y + Y, pl.x + X) is element (c, Y, X) of what hipdec_batch_to_tensor_oriented writes for the same entry
 *    (item, window, flip), orientation code, filter, dtype, scale and bias with desc->width / height replaced by pl.width / pl.height.  All four filters, all
 *    eight codes, all four dtypes and both layouts are taken; windows, flips and the size swap of quarter turns are that call's; whatever it refuses for a
 *    sample of pl.width x pl.height is refused here with the same status.
 *  - Everywhere else the canvas holds the fill element of its channel, with both fill domains exactly as in hipdec_batch_to_tensor_placed (fill NULL:
 *    component 0).  mask_dev (may be NULL): n_entries x height x width uint8, 1 outside the visible part and 0 inside it; every byte of it is written.
 *  - Every canvas element is written exactly once, and nothing outside out_dev's tensor and the mask is written.
 * A rectangle inside the canvas gives the bytes of hipdec_batch_to_tensor_placed.  places NULL: every rectangle is the whole canvas and the call is the
 * placed call with places NULL - with mask_dev NULL as well hipdec_batch_to_tensor_oriented, byte for byte and launch for launch.
 * Refused before a device is touched, HIPDEC_ERR_INVALID_ARGUMENT naming the entry: a non-positive side; an empty visible part; |x|, |y| or a side above
 * 2^24 (64-bit host arithmetic cannot overflow below it); a sample of pl.width x pl.height the oriented call's description check refuses.  Fills, domains,
 * `reserved`, out_bytes and codes are refused as the placed call refuses them.  pl.width * pl.height, or the canvas, above max_image_size_pixels:
 * HIPDEC_ERR_LIMIT.
 * Launches: ONE launch of the k_frame_* kernels - the oriented / resampling kernels with a clipping store - for all entries, and the margins and the mask in
 * ONE launch of k_canvas_margin over the visible rectangles (counted by hipdec_placed_stats' margin_launches); none when every visible part is its whole
 * canvas and no mask is asked for.  Work follows the visible part: the grid covers the pieces of work - a column tile of P x a block of rows (box: up to 96
 * columns for 8-bit and 64 for wider samples x 16 rows, or 64 / 32 rows for a quarter turn), a column tile x a band (bilinear / bicubic: up to 64 columns
 * x 16 rows of P), 256 x 4 displayed pixels (nearest) - from the first to the last one with a visible pixel along either axis; a piece with none loads no
 * source sample, and inside a piece the box filter accumulates the visible rows of P only.  No scratch memory, no intermediate.
 * CLIPS.  A frame of a clip is framed through the borrowed batch (hipdec_clips_batch, below) with no further code. */
HIPDEC_API int hipdec_batch_to_tensor_framed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_framed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
/* Host only, 64-bit integer arithmetic: the library's statement of torchvision's Resize(resize) -> CenterCrop((crop_height, crop_width)) on a DISPLAYED
 * sample of src_width x src_height, as the rectangle of a framed call whose canvas is the crop.  The shorter side becomes `resize`, the longer
 * floor(resize * long / short).  Per axis, with side the resized side and crop the crop's: side >= crop: offset = -roundhalfeven((side - crop) / 2) (Python's
 * round()); side < crop: offset = (crop - side) / 2 rounding down (the picture is padded, the smaller half in front).  A non-positive argument, or a side
 * above 2^24: -1, hipdec_last_error says why. */
HIPDEC_API int hipdec_resize_crop_place(int src_width, int src_height, int resize, int crop_width, int crop_height, hipdec_tensor_place* out);
/* counters since load: framed calls, their entries, and from the host's geometry the pieces of work (above) of entries with rectangles that held a visible
 * pixel and those that held none; tiles + tiles_skipped is the count of the unclipped samples */
HIPDEC_API void hipdec_framed_stats(uint64_t* calls, uint64_t* entries, uint64_t* tiles, uint64_t* tiles_skipped);

/* ---- composed tensor output: mosaic, CutMix and contact sheets - several samples in one canvas, one launch set ------------------------------------------
 * Mosaic-4 (the default augmentation of YOLOv5 / v8 / 11: four resized photos around a random centre, grey 114 elsewhere), CutMix (timm / DeiT / ConvNeXt:
 * a box of sample B pasted over sample A) and contact sheets / image grids (photo services, vision-language models that take an N x M sheet of letterboxed
 * thumbnails) all put SEVERAL samples into one picture.  Every other tensor form writes one sample per canvas; a host composing from them pays a round
 * trip or a pile of slice copies.  These calls map several entries to one canvas and decide who owns which pixel.
 *
 * THE DEFINITION OF THE RESULT.  The output is n_canvases x 3 x H x W (or NHWC) with desc->width x height the CANVAS; hipdec_tensor_bytes(desc, n_canvases)
 * is its size, and the mask (may be NULL) is n_canvases x H x W uint8.  Entry e belongs to canvas tiles[e].canvas.  tiles[e].place is the rectangle of its
 * resized, DISPLAYED sample in canvas coordinates and may leave the canvas on any side, as in the framed call.  tiles[e].clip is a rectangle of the canvas
 * the entry may write: clip.width == 0 && clip.height == 0 means the whole canvas (clip.x and clip.y are then not read); otherwise both sides are positive,
 * and it may leave the canvas too.  The entry's REGION is place n clip n canvas.  LATER ENTRIES LIE ON TOP: entry e OWNS the pixels of its region that lie
 * in no region of an entry j > e of the same canvas.
 *  - An owned canvas element (c, place.y + Y, place.x + X) is element (c, Y, X) of what hipdec_batch_to_tensor_oriented writes for that entry (item,
 *    window, flip), orientation code, filter, dtype, scale and bias with desc->width / height replaced by place.width / place.height.  All four filters, all
 *    eight codes, all four dtypes and both layouts are taken; whatever that call refuses for a sample of that size is refused here with the same status.
 *  - Pixels nobody owns hold the fill element of their channel, with both fill domains exactly as in hipdec_batch_to_tensor_placed (fill NULL: component
 *    0); the mask is 1 there and 0 on owned pixels.  A canvas without entries is all fill.
 *  - Every element of the tensor and of the mask is written exactly once, and nothing outside them is touched.
 * If every canvas has one entry with a whole-canvas clip and tiles[e].canvas == e, the bytes are those of hipdec_batch_to_tensor_framed.
 * Refused before a device is touched, HIPDEC_ERR_INVALID_ARGUMENT naming the entry: tiles NULL; n_entries or n_canvases below 1; a canvas outside
 * 0 .. n_canvases - 1; a non-positive side of place; a clip with one zero or a negative side; an empty region; |x|, |y| or a side above 2^24, of place or
 * of clip; more than HIPDEC_COMPOSE_MAX_ENTRIES entries in one canvas; out_bytes below hipdec_tensor_bytes(desc, n_canvases); fills, domains, `reserved`
 * and codes as the placed call refuses them.  HIPDEC_ERR_LIMIT: place.width * place.height, or the canvas, above max_image_size_pixels; the cover tables of
 * the call (below) above HIPDEC_COMPOSE_TABLE_BYTES; more than HIPDEC_COMPOSE_MAX_PIECES pieces.
 * An entry whose region later entries cover completely is legal: it records no work and counts in hidden_entries.
 * How it is done.  Per canvas the regions of later entries are subtracted from each entry's region, which leaves disjoint rectangles - PIECES (the rows
 * above the subtracted rectangle, those below it, and what lies left and right of it in between; the bytes do not depend on the decomposition).  Each piece
 * is one block of the k_frame_* kernels of the framed call: the sample's first element where it would lie in its canvas, the piece as the window.  ONE
 * launch of those kernels for all pieces of a call (a grid's z extent is 65535: more pieces take as few launches as that allows).  The fill and the mask
 * go out in ONE launch of k_compose_cover for all canvases: per canvas the union of all regions as a COVER TABLE - the ascending distinct row edges and, per
 * band of rows between two edges, the sorted, merged, disjoint covered column intervals; 2 * (bands + 1) + 2 * intervals 32-bit words - uploaded with the
 * per-canvas blocks in one copy.  No cover launch when no canvas has an unowned pixel and no mask is asked for.  No scratch memory, no intermediate.
 * CLIPS.  A clip's frame is composed through the borrowed batch (hipdec_clips_batch, below) with no further code. */
#define HIPDEC_COMPOSE_MAX_ENTRIES 256           /* entries of one canvas */
#define HIPDEC_COMPOSE_MAX_PIECES 65536          /* pieces of one call */
#define HIPDEC_COMPOSE_TABLE_BYTES (1u << 20)    /* cover tables of one call */
typedef struct hipdec_tensor_tile { int canvas; hipdec_tensor_place place; hipdec_tensor_place clip; } hipdec_tensor_tile;
HIPDEC_API int hipdec_batch_to_tensor_composed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                               const hipdec_tensor_tile* tiles, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, int n_canvases,
                                               void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_composed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                               const hipdec_tensor_tile* tiles, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, int n_canvases,
                                               void* out_dev, size_t out_bytes, void* stream);
/* The helpers below are host only, work in 64-bit integer arithmetic and return -1 with hipdec_last_error on bad arguments.
 * area[e]: the pixels entry e owns on a canvas of width x height, by the rules above (tiles are refused as the composed call refuses them).  CutMix's
 * lambda - the share of the base sample that stays visible - is exactly area[base] / (width * height). */
HIPDEC_API int hipdec_compose_visible_area(int width, int height, const hipdec_tensor_tile* tiles, int n_entries, int n_canvases, uint64_t* area);
/* The library's statement of YOLOv5's mosaic-4 rule: four DISPLAYED samples of widths[k] x heights[k], already resized, around the centre (xc, yc),
 * 0 < xc < canvas_w and 0 < yc < canvas_h, on canvas `canvas`.  Sample 0 has its bottom-right corner at the centre, sample 1 its bottom-left, sample 2 its
 * top-right, sample 3 its top-left; each is clipped to its quadrant (0: x < xc, y < yc; 1: x >= xc, y < yc; 2: x < xc, y >= yc; 3: x >= xc, y >= yc).
 * Sizes above 2^24 are refused. */
HIPDEC_API int hipdec_mosaic_tiles(int canvas_w, int canvas_h, int xc, int yc, const int* widths, const int* heights, int canvas, hipdec_tensor_tile* out);
/* A contact sheet of cols x rows cells of cell_w x cell_h with `gap` (>= 0) pixels between them, row-major: cell (r, c) is at (c * (cell_w + gap),
 * r * (cell_h + gap)) - the sheet is cols * cell_w + (cols - 1) * gap wide.  Entry k < n <= cols * rows, a DISPLAYED sample of widths[k] x heights[k], goes
 * into cell k through hipdec_letterbox_place(widths[k], heights[k], cell_w, cell_h, upscale, 1 (centre)), moved to the cell; its clip is the cell. */
HIPDEC_API int hipdec_sheet_tiles(int cols, int rows, int cell_w, int cell_h, int gap, const int* widths, const int* heights, int n, int upscale, int canvas,
                                  hipdec_tensor_tile* out);
/* counters since load: composed calls, their entries, the pieces recorded, the entries that were fully hidden, launches of k_compose_cover */
HIPDEC_API void hipdec_composed_stats(uint64_t* calls, uint64_t* entries, uint64_t* pieces, uint64_t* hidden_entries, uint64_t* cover_launches);

/* ---- packed tensor output: per-sample sizes and patch sequences in one launch ---------------------------------------------------------------------------
 * Native-resolution vision encoders (Qwen2-VL / 2.5-VL, SigLIP2 NaFlex, Pixtral, NaViT-style packing) take no common size: each photo keeps its aspect
 * ratio, is resized to its own w x h - a multiple of the patch size - and the batch is ONE packed sequence of patch tokens, [sum of tokens, 3 * P * P].
 * The tensor forms above take one desc->width x height for all entries and the placed form pads to one canvas; these calls take a size and an offset per
 * entry and write either dense samples or the patch sequence itself, all entries in one launch.  desc->width and desc->height must be 0 (the sizes are per
 * sample); dtype, layout, filter, scale and bias mean what they mean in the sibling calls.
 *
 * THE DEFINITION OF THE RESULT.  For entry e with samples[e] = (w, h, offset):
 *  - S[c][Y][X] is the element hipdec_batch_to_tensor_oriented writes at (c, Y, X) for the same entry (item, window, flip), orientation code, filter, dtype,
 *    scale and bias with desc->width / height = w / h.  Everything that call defines is untouched: integer stage, float stage, to-SDR rules, the size swap
 *    for an odd number of quarter turns, the flip of the displayed sample.
 *  - The sample occupies exactly the 3 * w * h elements out[offset .. offset + 3wh) (offset counts ELEMENTS of desc->dtype).
 *  - patch == 0, or patches NULL: the sample is stored densely in desc->layout,
 *      NCHW  out[offset + (c * h + Y) * w + X]          NHWC  out[offset + (Y * w + X) * 3 + c]
 *  - patch == P >= 1 with merge == m: w and h are multiples of P * m; with gw = w / P, gy = Y / P, gx = X / P, py = Y % P, px = X % P the token index is
 *      t = ((gy / m) * (gw / m) + gx / m) * m * m + (gy % m) * m + gx % m
 *    (m == 1: row-major gy * gw + gx; m == 2: the order Qwen2-VL's image processor emits), the position inside the token
 *      NCHW  k = (c * P + py) * P + px     the flattened Conv2d(3, D, P, P) weight order
 *      NHWC  k = (py * P + px) * 3 + c     NaFlex / big_vision patchify order
 *    and the element goes to out[offset + t * 3 * P * P + k].  As array expressions over the dense sample S (NCHW, shape [3, h, w], gh = h / P):
 *      m == 1, NHWC:  S.transpose(1, 2, 0).reshape(gh, P, gw, P, 3).transpose(0, 2, 1, 3, 4).reshape(gh * gw, P * P * 3)
 *      m == 2, NCHW:  S.reshape(3, gh / 2, 2, P, gw / 2, 2, P).transpose(1, 4, 2, 5, 0, 3, 6).reshape(gh * gw, 3 * P * P)
 * Every element of a sample's range is written exactly once and nothing else in `out` is written: gaps the caller leaves between samples stay as they were.
 * Entries of all sizes, codes and resampling-table sizes share one launch (65535 entries per launch, as in the siblings): ONE kernel launch for BOX and
 * NEAREST, one launch plus the one table upload of the resampling path for BILINEAR / BICUBIC.  Device time: slot [5] of hipdec_batch_slot_kernel_timing_us.
 * Refused before a device is touched, HIPDEC_ERR_INVALID_ARGUMENT, naming the entry where one is at fault: samples NULL; desc->width or height non-zero; a
 * sample with a non-positive side; patch < 0 or > 256; merge < 1 or > 16; merge != 1 with patch == 0; a non-zero `reserved`; a side that is not a multiple
 * of patch * merge; offset + 3wh above out_bytes / sizeof(element); two samples whose element ranges overlap; a code outside 0 .. 7; everything else the
 * oriented call refuses on its arguments alone.  w * h above max_image_size_pixels: HIPDEC_ERR_LIMIT.  What the oriented call refuses from the sources -
 * mixed 8-bit and wider entries, a float dtype from a source above 8 bits with BILINEAR / BICUBIC, resampling tables above 64 MiB - is refused with the same
 * status before anything is launched.
 * Out of scope: choosing the sizes stays with the caller, as reading `irot` does (Qwen's smart_resize and NaFlex's search over scales are float rules of
 * other projects); Qwen's duplicated temporal axis (hipdec_clips_to_tensor_packed below writes it); margins and masks (a packed sample has none); the single-image form. */
typedef struct hipdec_tensor_sample { int width, height; uint64_t offset; } hipdec_tensor_sample;   /* DISPLAYED size; index of the sample's first element in out */
typedef struct hipdec_tensor_patches { int patch, merge, reserved[2]; } hipdec_tensor_patches;      /* patch 0: dense samples; merge >= 1 */
HIPDEC_API int hipdec_batch_to_tensor_packed(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_packed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, void* out_dev,
                                             size_t out_bytes, void* stream);
/* Host only: offsets[e] of samples packed back to back in entry order, tokens[e] per sample ((w / patch) * (h / patch); 0 for dense samples) and the total
 * element count (any of the three may be NULL).  A refused argument - a bad `patches`, a non-positive side, a side that is no multiple of patch * merge -
 * returns -1 and hipdec_last_error says why. */
HIPDEC_API int hipdec_tensor_packed_layout(const hipdec_tensor_patches* patches, const int* widths, const int* heights, int n, uint64_t* offsets,
                                           uint32_t* tokens, uint64_t* total_elements);
/* counters since load: packed calls, their entries, and how many of those were written as patch sequences */
HIPDEC_API void hipdec_packed_stats(uint64_t* calls, uint64_t* entries, uint64_t* patch_entries);

/* ---- clips: the samples of several sequence tracks as ONE launch set, frames resident in device memory, video tensors ---------------------------------
 * A video loader wants a clip: T sampled frames of a track, one crop window and one flip for the whole clip, resized and normalised, as N x T x 3 x H x W,
 * N x 3 x T x H x W or token sequences.  A hipdec_clips object takes the samples of n_tracks tracks, decodes them as one launch set - the set the look-ahead
 * chains of hipdec_decoder objects share, built directly: no decoder objects, no coalescer - and keeps every picture in device memory; the tensor stage of
 * the batch calls above then serves its frames.
 *
 * SAMPLES.  Track t's samples are sample_counts[t] consecutive entries of samples[] / sample_sizes[] (track 0's first), in DECODING order, each one access
 * unit in the framing of hipdec_decoder_push_data ([u32 BE length][NAL]...).  A track's first sample carries the parameter sets and is a random-access
 * picture; later samples may repeat or replace parameter sets.  Each track starts from a fresh sequence state.
 * FRAMES.  The frames of a track are its output pictures in OUTPUT order - the order hipdec_decoder_next_picture releases them in with `flush`: coded video
 * sequence by coded video sequence (an IDR picture starts one), each in picture-order-count order.  Pictures with pic_output_flag == 0 are decoded but are
 * not frames; RASL pictures 8.3.3 drops are neither.  hipdec_clip_frame: `item` is the frame's item in the borrowed batch, `sample` the index of its sample
 * within the track, `poc` its picture order count, `sequence` the index of its coded video sequence within the track (from 0).
 * Refused by hipdec_clips_create before a device is touched, the message naming `track %d` (and `sample %d` where one is at fault): a NULL argument or a
 * non-positive count (HIPDEC_ERR_INVALID_ARGUMENT); broken framing (HIPDEC_ERR_END_OF_DATA); a sample that is not exactly one coded picture; more samples in
 * all than the chain limit (1024, HIPDEC_CHAIN_MAX_PICTURES: HIPDEC_ERR_LIMIT); and, with the status the front end gives, a sample it refuses, a first
 * sample without parameter sets, a P / B picture whose reference is not among the track's samples, 8-bit tracks beside wider ones.
 * hipdec_clips_run is asynchronous as hipdec_batch_run is, hipdec_clips_status synchronises as hipdec_batch_status does.
 * THE BORROWED BATCH.  hipdec_clips_batch returns the launch set as a hipdec_batch, valid until hipdec_clips_free: every hipdec_batch_* read, colour,
 * scaled, tensor, placed and packed call serves frames through it with item = hipdec_clip_frame.item.  hipdec_batch_run on it is refused with
 * HIPDEC_ERR_INVALID_ARGUMENT; hipdec_batch_free on it does nothing. */
typedef struct hipdec_clips hipdec_clips;
typedef struct hipdec_clip_frame { int item, sample, poc, sequence; hipdec_image_info info; } hipdec_clip_frame;
HIPDEC_API int hipdec_clips_create(hipdec_clips** out, int n_tracks, const int* sample_counts, const void* const* samples, const size_t* sample_sizes,
                                   uint64_t max_image_size_pixels);
HIPDEC_API void hipdec_clips_free(hipdec_clips* c);
HIPDEC_API int hipdec_clips_run(hipdec_clips* c, void* stream);
HIPDEC_API int hipdec_clips_status(hipdec_clips* c);
HIPDEC_API int hipdec_clips_track_count(const hipdec_clips* c);                /* a NULL object: HIPDEC_ERR_INVALID_ARGUMENT (negative) */
HIPDEC_API int hipdec_clips_frame_count(const hipdec_clips* c, int track);     /* a NULL object or a track outside the object's: HIPDEC_ERR_INVALID_ARGUMENT */
HIPDEC_API int hipdec_clips_frame(const hipdec_clips* c, int track, int frame, hipdec_clip_frame* out);
HIPDEC_API int hipdec_clips_frame_plane(hipdec_clips* c, int track, int frame, int plane, const void** dptr, size_t* stride);
HIPDEC_API int hipdec_clips_read_plane(hipdec_clips* c, int track, int frame, int plane, void* dst_host, size_t dst_stride);
HIPDEC_API hipdec_batch* hipdec_clips_batch(hipdec_clips* c);
/* counters since load: launch sets built, their tracks, their frames, clip tensor calls, and the frames that went through the strided box kernel */
HIPDEC_API void hipdec_clips_stats(uint64_t* sets, uint64_t* tracks, uint64_t* frames, uint64_t* tensor_calls, uint64_t* strided_box_entries);

/* CLIP TENSORS.  Entry e is a clip of T = clip->frames frames of track entries[e].item: frames[e * T + k], k = 0 .. T - 1, are frame indices of that track
 * (they may repeat and come in any order); the entry's window, flip and orientation code hold for all T frames.
 * THE DEFINITION OF THE RESULT.  F(e, k)[c][y][x] is, element for element, what hipdec_batch_to_tensor_oriented writes on the borrowed batch for the entry
 * (item of frame frames[e * T + k] of track entries[e].item, the entry's window and flip), the entry's code, and `desc` as given (filter, dtype, scale,
 * bias, width, height).  With W x H = desc->width x desc->height the output is n_entries * T * 3 * H * W elements without padding:
 *   HIPDEC_CLIP_FRAME_MAJOR,   NCHW  (N T C H W):  out[(((e * T + k) * 3 + c) * H + y) * W + x]
 *   HIPDEC_CLIP_FRAME_MAJOR,   NHWC  (N T H W C):  out[(((e * T + k) * H + y) * W + x) * 3 + c]
 *   HIPDEC_CLIP_CHANNEL_MAJOR, NCHW  (N C T H W):  out[(((e * 3 + c) * T + k) * H + y) * W + x]
 *   HIPDEC_CLIP_CHANNEL_MAJOR with NHWC: refused.
 * All four filters, all dtypes and all eight codes; the native-depth rule for float dtypes from sources above 8 bits and the refusal of floats from such
 * sources with BILINEAR / BICUBIC hold as in the oriented call.
 * Launches: BILINEAR / BICUBIC one launch plus its table upload, NEAREST one launch; BOX entries whose code with the flip folded in is 0 or 4 go through
 * the strided box kernel (the unoriented box kernel's stage with a row pitch and a plane stride), the other codes through the oriented box kernel: at most
 * two launches.  Device time: slot [5] of hipdec_batch_slot_kernel_timing_us of the borrowed batch.
 * Refused before the handle is read, HIPDEC_ERR_INVALID_ARGUMENT, naming the entry: `frames` NULL; T < 1; a non-zero `reserved`; temporal_patch > 1 (or
 * < 0); an unknown order; and - once the handle is read - a track or a frame index outside the object's.  Everything else as the oriented call refuses it.
 *
 * TOKEN SEQUENCES WITH A TEMPORAL PATCH (hipdec_clips_to_tensor_packed).  desc->width and height must be 0; samples[e] = (w, h, offset) is the displayed
 * size of clip e's frames and the element offset of the clip, which occupies exactly the 3 * T * w * h elements from there.
 *  - patch == 0 (or patches NULL): the clip is dense, in the orders above, at its own size; temporal_patch must be 0 or 1.
 *  - patch == P, merge == m, temporal_patch == Tp >= 1 (0 counts as 1): T % Tp == 0, the order is frame-major.  With gw = w / P, gh = h / P and gy, gx, py,
 *    px as in hipdec_batch_to_tensor_packed, the spatial token index is ts = ((gy / m) * (gw / m) + gx / m) * m * m + (gy % m) * m + gx % m, the token of the
 *    clip t = (k / Tp) * gh * gw + ts, the position inside the token
 *      NCHW  j = ((c * Tp + k % Tp) * P + py) * P + px          NHWC  j = (((k % Tp) * P + py) * P + px) * 3 + c
 *    and the element goes to out[offset + t * 3 * Tp * P * P + j].  For a clip S[T, 3, h, w] with Tp = 2, m = 2 (NCHW) this restates
 *      S.reshape(T/2, 2, 3, gh/2, 2, P, gw/2, 2, P).transpose(0, 3, 6, 4, 7, 2, 1, 5, 8).reshape(T/2 * gh * gw, 3 * 2 * P * P)
 *    the order Qwen2-VL's processor emits for video; a still becomes its image tokens with frames = {0, 0}.
 * Refused as the packed call refuses (the element range of a clip is 3 * T * w * h; overlap of two clips' ranges names the entry), and: T % Tp != 0;
 * Tp < 0 or Tp > 16; channel-major order with patches.
 * Out of scope: reading samples out of a container (stsz / ctts / moov parsing), choosing sizes, skipping the decode of pictures nobody sampled, audio, the
 * libheif hook, pipelining several hipdec_clips objects against each other. */
typedef enum { HIPDEC_CLIP_FRAME_MAJOR = 0, HIPDEC_CLIP_CHANNEL_MAJOR = 1 } hipdec_clip_order;
typedef struct hipdec_clip_desc { int frames /* T >= 1 */, order /* hipdec_clip_order */, temporal_patch /* 0 or 1 for dense clips */, reserved /* 0 */; } hipdec_clip_desc;
HIPDEC_API int hipdec_clips_to_tensor(hipdec_clips* c, const hipdec_tensor_desc* desc, const hipdec_clip_desc* clip, const hipdec_tensor_entry* entries,
                                      const int* frames, const int* orientations, int n_entries, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_clips_to_tensor_packed(hipdec_clips* c, const hipdec_tensor_desc* desc, const hipdec_clip_desc* clip, const hipdec_tensor_entry* entries,
                                             const int* frames, const int* orientations, const hipdec_tensor_sample* samples,
                                             const hipdec_tensor_patches* patches, int n_entries, void* out_dev, size_t out_bytes, void* stream);
/* Host only, the clip form of hipdec_tensor_packed_layout: offsets[e] of clips of `frames` frames packed back to back in entry order (3 * frames * w * h
 * elements each), tokens[e] per clip ((frames / Tp) * (w / patch) * (h / patch); 0 for dense clips) and the total element count (any of the three may be
 * NULL).  A refused argument returns -1 and hipdec_last_error says why. */
HIPDEC_API int hipdec_clip_packed_layout(const hipdec_clip_desc* clip, const hipdec_tensor_patches* patches, const int* widths, const int* heights, int n,
                                         uint64_t* offsets, uint32_t* tokens, uint64_t* total_elements);

/* ---- warped tensor output: Pillow-exact affine transforms of the resized 8-bit picture, normalised, in one call ------------------------------------------
 * RandomRotation, RandomAffine, the geometric operations of RandAugment / AutoAugment / TrivialAugment (Rotate, ShearX/Y, TranslateX/Y) and the scale and
 * translate jitter of detection loaders are, in the libraries people train with, PIL.Image.transform(size, AFFINE, data, resample, fillcolor) applied to the
 * already resized 8-bit picture.  The warp stage does exactly that to 8-bit interleaved RGB samples in device memory - per sample one map and one fill - and
 * writes the normalised tensor the other tensor calls write.
 *
 * THE STAGE (hipdec_tensor_warp).  S is a source sample of sh x sw x 3 bytes (sw = src_width, sh = src_height), a = maps[e].m[0 .. 5] (PIL's AFFINE data:
 * the centre of an output pixel to source coordinates).  All arithmetic is IEEE double, one rounding per written operation, no fused multiply-add, evaluated
 * left to right.  FLOOR(v) = (int)floor(v) for v < 0, else (int)v.  COORD(v) = -1 for v < 0, else (int)v.  An output pixel that is "outside" holds the fill.
 *  HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC, output pixel (x, y) of the desc->width x desc->height sample:
 *    xin = a0 * (x + 0.5) + a1 * (y + 0.5) + a2,  yin = a3 * (x + 0.5) + a4 * (y + 0.5) + a5;  outside if xin < 0 || xin >= sw || yin < 0 || yin >= sh;
 *    else xin -= 0.5, yin -= 0.5, ix = FLOOR(xin), iy = FLOOR(yin), dx = xin - ix, dy = yin - iy.  Columns are clamped to [0, sw - 1].
 *    Bilinear: L(p, q, d) = p + (q - p) * d;  v1 = L over columns ix, ix + 1 of row clamp(iy);  v2 the same over row iy + 1 if 0 <= iy + 1 < sh, else v1;
 *              V = (uint8)L(v1, v2, dy), truncating.
 *    Bicubic:  B(v1, v2, v3, v4, d): p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4, result p1 + d * (p2 + d * (p3 + d * p4)).
 *              A row's value is B over columns ix - 1 .. ix + 2 with dx.  Row iy - 1 is clamped; rows iy, iy + 1, iy + 2 are each used only if inside
 *              [0, sh), else they repeat the previous row's value.  v = B of the four row values with dy;  V = 0 if v <= 0, 255 if v >= 255, else (uint8)v.
 *  HIPDEC_SCALE_NEAREST with a1 == 0 && a3 == 0 (Pillow's scale path): the host builds xt[x] = COORD(xo), xo starting at a2 + a0 * 0.5 and xo += a0 after
 *    each x - a running sum -, and yt[y] likewise from a5, a4.  V = S[yt[y]][xt[x]]; outside if a table value is not inside the source.
 *  HIPDEC_SCALE_NEAREST otherwise (Pillow's fixed-point path): FIX(v) = FLOOR(v * 65536.0 + 0.5);  A0 = FIX(a0), A1 = FIX(a1), A3 = FIX(a3), A4 = FIX(a4),
 *    A2 = FIX(a2 + a0 * 0.5 + a1 * 0.5), A5 = FIX(a5 + a3 * 0.5 + a4 * 0.5);  column (A2 + y * A1 + x * A0) >> 16, row (A5 + y * A4 + x * A3) >> 16
 *    (arithmetic shifts); outside if either is not inside the source.
 *  HIPDEC_SCALE_BOX has no warp and is refused.
 * Float stage, dtypes and layouts: those of hipdec_batch_to_tensor with V the 8-bit component value; desc->filter is not read by hipdec_tensor_warp.
 * fill: hipdec_tensor_fill as in the placed call - HIPDEC_FILL_COMPONENT (an integer 0 .. 255) is normalised as a pixel is, HIPDEC_FILL_ELEMENT is stored
 * as it is; NULL: component 0.  There is no mask output.
 * src_dev: n dense samples back to back (NHWC), src_bytes at least n * sh * sw * 3.  n == 0 is allowed: nothing is launched, nothing is counted.
 *
 * THE DECODE-SIDE FORMS (hipdec_batch_to_tensor_warped, hipdec_album_to_tensor_warped).  Sample e of the intermediate is, byte for byte, what
 * hipdec_batch_to_tensor_oriented writes for entry e (item, window, flip) and orientations[e] with dtype U8, layout NHWC, size src_width x src_height and
 * desc->filter - the RESIZE filter, all four allowed; then the stage above with warp->filter.  The identity map with src_width x src_height equal to
 * desc->width x height gives hipdec_batch_to_tensor_oriented's bytes.  A float dtype from a source above 8 bits is HIPDEC_ERR_UNSUPPORTED, as for the
 * Pillow resize filters; U8 goes through to-SDR.  The intermediate of n * sh * sw * 3 bytes comes from the library's device pool; the handle keeps it for
 * its next warped call and returns it to the pool when it is freed.  The inner resize counts in hipdec_tensor_stats and hipdec_oriented_stats as the
 * oriented call does.
 *
 * Launches: the existing resize launch (decode-side forms), then ALL entries through ONE launch of k_warp, whatever their number; the maps may all differ.
 * Asynchronous on `stream`.  Refused with HIPDEC_ERR_INVALID_ARGUMENT before anything is launched, `out_dev` untouched, the entry named: a non-finite
 * coefficient; |m[i]| >= 32000; a corner of [0, width] x [0, height] whose mapped coordinate has magnitude >= 32000 (stricter than Pillow's own 32768, so
 * that Pillow always takes the paths above and the fixed-point sums cannot wrap); and for the call: src_width or src_height < 1 or >= 32768, an unknown
 * warp filter or BOX, a non-zero `reserved`, a fill the placed call refuses or a component fill above 255, src_bytes or out_bytes too small.  More than
 * 2^31 - 1 output tiles (64 x 16 pixels) in a call: HIPDEC_ERR_LIMIT.
 * Not part of it: perspective and quad transforms (hipdec_tensor_project below); expand (pass a larger size); a mask (the point-wise RandAugment operations are the photo stage below,
 * hipdec_tensor_photo: chain the two through a U8 / NHWC buffer); a clips entry point (repeat
 * the map for the T frames of a clip and use hipdec_tensor_warp); Lanczos; warping straight from the full-size picture in one resampling. */
typedef struct hipdec_tensor_map { double m[6]; } hipdec_tensor_map;
typedef struct hipdec_warp_desc {
  int src_width, src_height;   /* size of the intermediate picture the maps read */
  int filter;                  /* HIPDEC_SCALE_NEAREST, _BILINEAR or _BICUBIC */
  int reserved;                /* 0 */
} hipdec_warp_desc;
HIPDEC_API int hipdec_tensor_warp(const void* src_dev, size_t src_bytes, const hipdec_warp_desc* warp, const hipdec_tensor_map* maps,
                                  const hipdec_tensor_fill* fill, const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_tensor_warped(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_warp_desc* warp, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, int n_entries,
                                             void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_warped(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_warp_desc* warp, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, int n_entries,
                                             void* out_dev, size_t out_bytes, void* stream);
/* Host only.  The map PIL.Image.rotate(angle) - counter-clockwise degrees about the centre, no expand - hands to its AFFINE transform for a picture of
 * width x height: the angle mod 360, cos and sin of -radians(angle) rounded to 15 decimal places, centre (width / 2, height / 2), the translation as
 * Pillow computes it.  A non-finite angle, a non-positive size or out NULL: -1, hipdec_last_error says why. */
HIPDEC_API int hipdec_rotate_map(double angle, int width, int height, hipdec_tensor_map* out);
/* counters since load: launches of k_warp - one per call that wrote anything - and the entries they wrote */
HIPDEC_API void hipdec_warp_stats(uint64_t* calls, uint64_t* entries);

/* ---- projective tensor output: Pillow-exact PERSPECTIVE and QUAD transforms of the resized 8-bit picture, normalised, in one call ----------------------------
 * torchvision's RandomPerspective and F.perspective, the keystone jitter of OCR / document / scene-text loaders (PERSPECTIVE) and the rectification of a
 * photographed page from its four corners (QUAD) are PIL.Image.transform(size, PERSPECTIVE | QUAD, data, resample, fillcolor) applied to the already resized
 * 8-bit picture.  The projective stage does exactly that to 8-bit interleaved RGB samples in device memory - per sample one map and one fill - and writes the
 * normalised tensor the other tensor calls write.  Bit-equal to Pillow, no tolerance.
 *
 * THE STAGE (hipdec_tensor_project).  S, sw, sh, FLOOR, COORD and "outside" as in hipdec_tensor_warp above.  A map is eight doubles a = maps[e].a[0 .. 7] and
 * a kind.  For output pixel (x, y) of the desc->width x desc->height sample let xc = (double)x + 0.5 and yc = (double)y + 0.5.  Every written operator is one
 * IEEE double operation with one rounding, evaluated left to right in this order; no fused multiply-add; the division is the IEEE division.
 *  HIPDEC_PROJECT_PERSPECTIVE: xin = (a0 * xc + a1 * yc + a2) / (a6 * xc + a7 * yc + 1.0),  yin = (a3 * xc + a4 * yc + a5) / (a6 * xc + a7 * yc + 1.0);
 *    a is Pillow's PERSPECTIVE data as given (hipdec_perspective_map makes it from four point pairs).
 *  HIPDEC_PROJECT_QUAD:        xin = a0 + a1 * xc + a2 * yc + a3 * xc * yc,  yin = a4 + a5 * xc + a6 * yc + a7 * xc * yc;
 *    a is what Pillow's Python layer makes of the four corners (hipdec_quad_map).
 *  warp->filter HIPDEC_SCALE_NEAREST: sx = COORD(xin), sy = COORD(yin); outside if sx < 0 || sx >= sw || sy < 0 || sy >= sh, else V = S[sy][sx].  This is
 *    Pillow's generic per-pixel path - NOT the fixed-point path or the running-sum tables of the AFFINE call, which hipdec_tensor_warp states: a PERSPECTIVE
 *    map with a6 = a7 = 0 and NEAREST need not give hipdec_tensor_warp's bytes for m = a[0 .. 5] (Pillow's own two methods differ there).
 *  HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC: from (xin, yin) on exactly the statements of hipdec_tensor_warp - outside if xin < 0 || xin >= sw || yin < 0
 *    || yin >= sh, else xin -= 0.5, yin -= 0.5, FLOOR, dx, dy, the clamped columns, the rows used only where they exist, L and B, the truncation or the clamp
 *    to 0 .. 255.  A PERSPECTIVE map with a6 = a7 = 0 therefore gives hipdec_tensor_warp's bytes for m = a[0 .. 5]: a division by exactly 1.0 is exact.
 *  HIPDEC_SCALE_BOX is refused.  warp is the hipdec_warp_desc of the warped call: the source size and the filter.  Entries of one call may mix the kinds.
 * Float stage, dtypes, layouts, fill (hipdec_tensor_fill, component or element domain; NULL: component 0), src_dev / src_bytes and n == 0: as in
 * hipdec_tensor_warp.  With a U8 / NHWC output the stage chains with hipdec_tensor_warp, hipdec_tensor_photo, hipdec_tensor_augment and hipdec_tensor_recipe.
 *
 * THE DECODE-SIDE FORMS (hipdec_batch_to_tensor_projected, hipdec_album_to_tensor_projected): the warped forms with this stage.  Sample e of the intermediate
 * is what hipdec_batch_to_tensor_oriented writes for entry e and orientations[e] with dtype U8, layout NHWC, size src_width x src_height and desc->filter;
 * then the stage above.  A float dtype from a source above 8 bits is HIPDEC_ERR_UNSUPPORTED.  The intermediate is the one the handle keeps for its warped
 * calls.  The inner resize counts in hipdec_tensor_stats and hipdec_oriented_stats; the call counts in hipdec_project_stats, not in hipdec_warp_stats.
 *
 * Launches: the existing resize launch (decode-side forms), then ALL entries through ONE launch of k_project, whatever their number, kinds and maps.
 * Asynchronous on `stream`.  Refused with HIPDEC_ERR_INVALID_ARGUMENT before any device is touched, `out_dev` untouched, naming `entry %d`: a kind other than
 * 0 or 1; a non-zero `reserved`; a non-finite coefficient; |a[i]| >= 32000; at a corner of [0, width] x [0, height] a mapped coordinate of magnitude >= 32000
 * or, for PERSPECTIVE, a denominator a6 * cx + a7 * cy + 1.0 below 1.0 / 1048576.  The corners decide for every pixel centre: the denominator is linear, a
 * linear-fractional map over a region of positive denominator and a bilinear map take their extremes at the vertices, and the floor of 2^-20 keeps rounding
 * from turning a positive denominator into zero - so Pillow sees no NaN and no integer overflow and never leaves the paths stated above.  And for the call:
 * everything hipdec_tensor_warp refuses of the desc, the warp desc, the fill, n, the byte counts; more than 2^31 - 1 tiles: HIPDEC_ERR_LIMIT.
 * Not part of it: a projective step inside recipe chains; MESH; a mask; expand; a clips entry point (repeat the map for the T frames of a clip). */
#define HIPDEC_PROJECT_PERSPECTIVE 0
#define HIPDEC_PROJECT_QUAD        1
typedef struct hipdec_tensor_projection { double a[8]; int kind; int reserved; } hipdec_tensor_projection;
HIPDEC_API int hipdec_tensor_project(const void* src_dev, size_t src_bytes, const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps,
                                     const hipdec_tensor_fill* fill, const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_tensor_projected(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                                const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill,
                                                int n_entries, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_projected(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                                const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill,
                                                int n_entries, void* out_dev, size_t out_bytes, void* stream);
/* Host only.  The PERSPECTIVE map that sends endpoints[k] (output coordinates) to startpoints[k] (source coordinates), k = 0 .. 3, x, y pairs - the library's
 * statement of torchvision's _get_perspective_coeffs (torchvision is not installed where the library is tested, and not pinned): per pair the rows
 * [ex, ey, 1, 0, 0, 0, -sx * ex, -sx * ey | sx] and [0, 0, 0, ex, ey, 1, -sy * ex, -sy * ey | sy], the 8 x 8 system solved in double by Gaussian elimination
 * with partial pivoting.  A singular system, a non-finite point or a NULL argument: HIPDEC_ERR_INVALID_ARGUMENT. */
HIPDEC_API int hipdec_perspective_map(const double startpoints[8], const double endpoints[8], hipdec_tensor_projection* out);
/* Host only.  The QUAD map of Image.transform((width, height), QUAD, corners) as Pillow's Python layer computes it, operator for operator: corners = (nw, sw,
 * se, ne) as x, y pairs in source coordinates, As = 1.0 / width, At = 1.0 / height (the OUTPUT size); a0 = nw.x, a1 = (ne.x - nw.x) * As,
 * a2 = (sw.x - nw.x) * At, a3 = (se.x - sw.x - ne.x + nw.x) * As * At; a4 .. a7 the same in y.  A non-finite corner, a non-positive size or a NULL argument:
 * HIPDEC_ERR_INVALID_ARGUMENT. */
HIPDEC_API int hipdec_quad_map(const double corners[8], int width, int height, hipdec_tensor_projection* out);
/* counters since load: launches of k_project - one per call that wrote anything - and the entries they wrote */
HIPDEC_API void hipdec_project_stats(uint64_t* calls, uint64_t* entries);

/* ---- photometric tensor output: Pillow-exact ColorJitter / RandAugment colour operations on the resized 8-bit picture, normalised --------------------------
 * ColorJitter (brightness, contrast, saturation), RandomGrayscale, the colour half of RandAugment / AutoAugment / TrivialAugment (Brightness, Color,
 * Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize, Invert) and RandomAdjustSharpness / RandomAutocontrast / RandomEqualize /
 * RandomPosterize / RandomSolarize / RandomInvert are, in the libraries people train with, PIL.ImageEnhance.* and PIL.ImageOps.* calls on the already resized
 * 8-bit picture.  The photo stage does exactly that to 8-bit interleaved RGB samples in device memory - per sample a chain of up to HIPDEC_PHOTO_MAX_OPS
 * operations - and writes the normalised tensor the other tensor calls write.  Bit-equal to Pillow, no tolerance.
 *
 * THE STAGE (hipdec_tensor_photo).  S is a sample of h x w x 3 bytes (w = src_width, h = src_height), V one of its components.  The operations of
 * chains[e] are applied in order, each to the 8-bit result of the one before it; an empty chain is the identity.
 *  BLEND(D, V, f) - PIL.Image.blend(degenerate, image, f) per component: alpha = (float)f;  t = (float)D + alpha * (float)(V - D) in IEEE single precision,
 *    the product rounded, then the sum (no fused multiply-add: the library is built with -ffp-contract=off, and this definition depends on it).
 *    If 0 <= alpha <= 1 the result is (uint8)t, truncating; otherwise 0 if t <= 0, 255 if t >= 255, else (uint8)t.
 *  LUM(R, G, B) = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 - convert("L").
 *  HIPDEC_PHOTO_BRIGHTNESS (value f)  BLEND(0, V, f)                                                          ImageEnhance.Brightness
 *  HIPDEC_PHOTO_COLOR (f)             BLEND(LUM of the pixel, V, f); f = 0 is RandomGrayscale / convert("L") exactly   ImageEnhance.Color
 *  HIPDEC_PHOTO_CONTRAST (f)          BLEND(m, V, f), m = (int)((double)(sum of LUM over the sample) / (double)(w * h) + 0.5)   ImageEnhance.Contrast
 *  HIPDEC_PHOTO_SHARPNESS (f)         BLEND(SM, V, f), SM the sample through ImageFilter.SMOOTH:                ImageEnhance.Sharpness
 *      interior pixels (uint8)clip(((0.5f + row(y - 1)) + row(y)) + row(y + 1)) in single precision - the top row first -, clip(s) = 0 if s <= 0, 255 if
 *      s >= 255;  row(r) = (S[r][x - 1] * k + S[r][x] * c) + S[r][x + 1] * k with k = (float)(1.0 / 13) and c = (float)(5.0 / 13) for r = y, c = k for the
 *      rows above and below (the kernel 1 1 1 / 1 5 1 / 1 1 1 over 13).  Border pixels - the first and last row and column, every pixel when w < 3 or
 *      h < 3 - are S.
 *  HIPDEC_PHOTO_POSTERIZE (value an integer 0 .. 8)   V & ((0xFF << (8 - bits)) & 0xFF)                        ImageOps.posterize
 *  HIPDEC_PHOTO_SOLARIZE (threshold t, a double)      V if (double)V < t, else 255 - V                          ImageOps.solarize
 *  HIPDEC_PHOTO_INVERT                                255 - V                                                   ImageOps.invert
 *  HIPDEC_PHOTO_AUTOCONTRAST   per channel: lo, hi the least and greatest value present; hi <= lo: identity; else scale = 255.0 / (hi - lo),
 *      offset = -lo * scale in double and V' = clamp((int)(V * scale + offset), 0, 255): one rounding per operation, no contraction, truncation toward
 *      zero.                                                                                                    ImageOps.autocontrast, cutoff 0
 *  HIPDEC_PHOTO_EQUALIZE       per channel with histogram H: fewer than two non-zero bins: identity; step = (w * h - H[last non-zero bin]) / 255 (integer);
 *      step == 0: identity; else V' = min(255, (step / 2 + H[0] + .. + H[V - 1]) / step) (integer).            ImageOps.equalize
 * The value of an operation that takes none is not read beyond the checks below (pass 0).
 * Float stage, dtypes and layouts: those of hipdec_batch_to_tensor with V the 8-bit component value.  desc->width x height must equal the source size - the
 * stage does not resize - and desc->filter is not read.  HIPDEC_TENSOR_U8 with HIPDEC_TENSOR_NHWC writes samples of the stage's own input format, so the
 * stage chains with hipdec_tensor_warp in either order through such a buffer.
 * src_dev: n dense samples back to back (NHWC), src_bytes at least n * h * w * 3; it is not written.  n == 0 is allowed: nothing is launched or counted.
 * A clip's frames share a chain by repeating it; CONTRAST's mean is then per frame, as in the host recipes.
 *
 * THE DECODE-SIDE FORMS (hipdec_batch_to_tensor_photo, hipdec_album_to_tensor_photo).  Sample e of the intermediate is, byte for byte, what
 * hipdec_batch_to_tensor_oriented writes for entry e and orientations[e] with dtype U8, layout NHWC, size src_width x src_height and desc->filter (all four
 * resize filters, windows, flips, codes); then the stage above.  An empty chain for every entry gives hipdec_batch_to_tensor_oriented's bytes.  A float
 * dtype from a source above 8 bits is HIPDEC_ERR_UNSUPPORTED, as for the warp; U8 goes through to-SDR.  The intermediate, the stage's ping-pong buffers
 * and histograms come from the library's device pool; the handle keeps them for its next photo call and returns them when it is freed.  The inner resize
 * counts in hipdec_tensor_stats and hipdec_oriented_stats as the oriented call does.
 *
 * Launches: the existing resize launch (decode-side forms); then per chain step at most ONE launch of k_photo_hist - only if an entry's operation at that
 * step is CONTRAST, AUTOCONTRAST or EQUALIZE - and ONE of k_photo_apply, whatever the number of entries: at most 2 * HIPDEC_PHOTO_MAX_OPS.  Chains of
 * different lengths and operations share the launches; they are aligned at their first operation.  The statistics never leave the device.
 * Asynchronous on `stream`.  Refused with HIPDEC_ERR_INVALID_ARGUMENT before anything is launched, `out_dev` untouched, the entry and the operation
 * named: n_ops outside 0 .. HIPDEC_PHOTO_MAX_OPS; an unknown op; a non-zero `reserved`; a value that is not finite or has |value| > 65536; POSTERIZE with a
 * value that is not an integer 0 .. 8; and for the call: src_width or src_height < 1 or >= 32768, a desc size that is not the source size, an unknown dtype
 * or layout, a non-finite scale or bias, src_bytes or out_bytes too small, more than 2^31 - 1 tiles (64 x 16 pixels).
 * Not part of it: gamma; autocontrast cutoffs and masks; parameter samplers; a clips entry point.  Hue, Gaussian blur and chains of more than four
 * operations are the augment stage below (hipdec_tensor_augment); a photometric and a warp step inside one call is the recipe stage
 * (hipdec_tensor_recipe). */
#define HIPDEC_PHOTO_MAX_OPS 4
typedef enum hipdec_photo_opcode {
  HIPDEC_PHOTO_BRIGHTNESS = 1, HIPDEC_PHOTO_COLOR = 2, HIPDEC_PHOTO_CONTRAST = 3, HIPDEC_PHOTO_SHARPNESS = 4, HIPDEC_PHOTO_POSTERIZE = 5,
  HIPDEC_PHOTO_SOLARIZE = 6, HIPDEC_PHOTO_INVERT = 7, HIPDEC_PHOTO_AUTOCONTRAST = 8, HIPDEC_PHOTO_EQUALIZE = 9
} hipdec_photo_opcode;
typedef struct hipdec_photo_op {
  int op;                      /* hipdec_photo_opcode */
  int reserved;                /* 0 */
  double value;                /* the factor f, the bits, the threshold; 0 for INVERT, AUTOCONTRAST, EQUALIZE */
} hipdec_photo_op;
typedef struct hipdec_photo_chain {
  int n_ops;                   /* 0 .. HIPDEC_PHOTO_MAX_OPS */
  int reserved;                /* 0 */
  hipdec_photo_op ops[HIPDEC_PHOTO_MAX_OPS];
} hipdec_photo_chain;
typedef struct hipdec_photo_desc {
  int src_width, src_height;   /* size of the samples: the intermediate picture of the decode-side forms */
  int reserved[2];             /* 0 */
} hipdec_photo_desc;
HIPDEC_API int hipdec_tensor_photo(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_photo_chain* chains,
                                   const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_tensor_photo(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                            const hipdec_photo_desc* photo, const hipdec_photo_chain* chains, int n_entries, void* out_dev, size_t out_bytes,
                                            void* stream);
HIPDEC_API int hipdec_album_to_tensor_photo(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                            const hipdec_photo_desc* photo, const hipdec_photo_chain* chains, int n_entries, void* out_dev, size_t out_bytes,
                                            void* stream);
/* counters since load: photo calls that wrote anything, the entries they wrote, and the launches of k_photo_hist and k_photo_apply together */
HIPDEC_API void hipdec_photo_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches);

/* ---- augmented tensor output: the photo stage's operations plus Pillow-exact hue and Gaussian blur, chains of up to eight --------------------------------
 * The self-supervised and contrastive recipes (SimCLR, MoCo v2 / v3, BYOL, SwAV, DINO / iBOT / DINOv2) are ColorJitter(brightness, contrast, saturation,
 * hue) -> RandomGrayscale -> PIL.ImageFilter.GaussianBlur(radius) -> Solarize per crop: up to seven steps, two of which the photo stage does not have.  The
 * augment stage is the photo stage with those two operations and chains of up to HIPDEC_AUGMENT_MAX_OPS.  Bit-equal to Pillow, no tolerance.
 *
 * THE STAGE (hipdec_tensor_augment).  As hipdec_tensor_photo, word for word: S is a sample of h x w x 3 bytes, the operations of chains[e] are applied in
 * order, each to the 8-bit result of the one before it, an empty chain is the identity; the float stage, dtypes, layouts, src_dev / src_bytes, n == 0, and
 * desc's size being the source size are the photo stage's; U8 / NHWC output chains with hipdec_tensor_warp, hipdec_tensor_photo and this call.  Opcodes
 * 1 .. 9 are hipdec_photo_opcode with exactly the photo stage's definitions, value checks and refusals: a chain of at most HIPDEC_PHOTO_MAX_OPS of them
 * gives hipdec_tensor_photo's bytes.  The two further operations:
 *  HIPDEC_AUGMENT_HUE (value: the shift d, an integer 0 .. 255)   per pixel (H, S, V) = rgb2hsv(R, G, B); H' = (H + d) & 255; hsv2rgb(H', S, V) -
 *    convert("HSV"), a uint8 wrap-around add on H, convert("RGB"): what torchvision's PIL adjust_hue does with d = (int)(hue_factor * 255) mod 256.
 *    rgb2hsv: mx, mn the greatest and least component; V = mx.  mx == mn: H = S = 0.  Otherwise, in float unless a double constant is written:
 *      cr = (float)(mx - mn); s = cr / (float)mx; rc = (float)(mx - R) / cr, gc and bc alike;
 *      R == mx: h = bc - gc;  else G == mx: h = (float)(2.0 + (double)rc - (double)bc);  else h = (float)(4.0 + (double)gc - (double)rc);
 *      h = (float)fmod((double)h / 6.0 + 1.0, 1.0);  H = clip8((int)((double)h * 255.0)), S = clip8((int)((double)s * 255.0)).
 *    hsv2rgb: S == 0: R = G = B = V.  Otherwise hf = (double)(float)H * 6.0 / 255.0; i = (int)floor(hf); f = (float)(hf - (double)(float)i);
 *      fs = (float)((double)S / 255.0); with round() half away from zero and every result clipped to 0 .. 255:
 *      p = round(V * (1.0 - (double)fs)); q = round(V * (1.0 - (double)(fs * f))) - the product fs * f in float -;
 *      t = round(V * (1.0 - (double)fs * (1.0 - (double)f))) - all in double -;
 *      (R, G, B) by i % 6: 0 (V, t, p); 1 (q, V, p); 2 (p, V, t); 3 (p, q, V); 4 (t, p, V); 5 (V, p, q).  (H = 255 gives i = 6: case 0.)
 *    Single-precision divisions are correctly rounded, one rounding per written operation (no fast-math, -ffp-contract=off).
 *  HIPDEC_AUGMENT_GAUSSIAN_BLUR (value: Pillow's radius rho, 0 <= rho <= HIPDEC_AUGMENT_BLUR_MAX_RADIUS)   ImageFilter.GaussianBlur(rho): three extended box
 *    blurs along rows, then three along columns, of all three channels, each pass on the 8-bit result of the one before.  The box (hipdec_gaussian_box), in
 *    single precision with one rounding per operation: sigma2 = rho * rho / 3; L = (float)sqrt(12.0 * (double)sigma2 + 1.0);
 *      l = (float)floor(((double)L - 1.0) / 2.0); a = (2 l + 1) * (l * (l + 1) - 3 * sigma2); a = a / (6 * (sigma2 - (l + 1) * (l + 1))); fr = l + a;
 *      r = (int)fr; ww = (uint32)((float)(1 << 24) / (fr * 2 + 1)); fw = ((1 << 24) - (2 r + 1) * ww) / 2.
 *    One pass over a line of n samples, c(i) = min(max(i, 0), n - 1), in 32-bit unsigned arithmetic:
 *      out[x] = (ww * (in[c(x - r)] + .. + in[c(x + r)]) + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + (1 << 23)) >> 24.
 *    rho = 0 is the identity; the cap gives r <= 7.
 *
 * THE DECODE-SIDE FORMS (hipdec_batch_to_tensor_augmented, hipdec_album_to_tensor_augmented): as the _photo forms - sample e of the intermediate is what
 * hipdec_batch_to_tensor_oriented writes for entry e as U8 / NHWC of size src_width x src_height with desc->filter; an empty chain for every entry gives
 * that call's bytes; a float dtype from a source above 8 bits is HIPDEC_ERR_UNSUPPORTED; the intermediate and the work memory come from the library's
 * device pool and stay with the handle.
 *
 * Launches: the existing resize launch (decode-side forms); then per chain step at most ONE launch each of k_photo_hist, k_photo_apply, k_augment_hue and
 * k_augment_blur, each over the entries whose operation at that step is of its kind (an empty chain's identity step is k_photo_apply's): at most
 * 4 * HIPDEC_AUGMENT_MAX_OPS, whatever the number of entries.  Chains are aligned at their first operation.  The blur's six passes are one launch: a
 * workgroup stages its 64 x 32 tile and a halo of 3 (r + 1) pixels in LDS and no intermediate goes through memory; entries of one launch may have
 * different radii.  Asynchronous on `stream`.  hipdec_photo_stats does not move for these calls.
 * Refused with HIPDEC_ERR_INVALID_ARGUMENT before anything is launched and before a device is touched, `out_dev` untouched, the entry and the operation
 * named: what hipdec_tensor_photo refuses (with HIPDEC_AUGMENT_MAX_OPS for the chain length); an op other than 1 .. 9, 16, 17 ("unknown op"); HUE with a
 * value that is not an integer 0 .. 255; GAUSSIAN_BLUR with a radius that is not finite, negative or above the cap; more than 2^31 - 1 tiles.
 * Not part of it: per-axis radii, BoxBlur, UnsharpMask; torchvision's tensor-path GaussianBlur(kernel_size, sigma), a different filter; gamma; parameter
 * samplers and the random order of ColorJitter's steps (the caller orders the chain); a clips entry point.  A warp step inside the chain is the recipe stage below
 * (hipdec_tensor_recipe). */
#define HIPDEC_AUGMENT_MAX_OPS 8
#define HIPDEC_AUGMENT_HUE 16            /* value: integer shift d, 0 .. 255 */
#define HIPDEC_AUGMENT_GAUSSIAN_BLUR 17  /* value: Pillow's radius, 0 <= radius <= HIPDEC_AUGMENT_BLUR_MAX_RADIUS */
#define HIPDEC_AUGMENT_BLUR_MAX_RADIUS 8.0
typedef struct hipdec_augment_chain {
  int n_ops;                   /* 0 .. HIPDEC_AUGMENT_MAX_OPS */
  int reserved;                /* 0 */
  hipdec_photo_op ops[HIPDEC_AUGMENT_MAX_OPS];   /* op: hipdec_photo_opcode, HIPDEC_AUGMENT_HUE or HIPDEC_AUGMENT_GAUSSIAN_BLUR */
} hipdec_augment_chain;
HIPDEC_API int hipdec_tensor_augment(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_augment_chain* chains,
                                     const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_tensor_augmented(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                                const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, int n_entries, void* out_dev,
                                                size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_augmented(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                                const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, int n_entries, void* out_dev,
                                                size_t out_bytes, void* stream);
/* counters since load: augment calls that wrote anything, the entries they wrote, and all kernel launches of the stage */
HIPDEC_API void hipdec_augment_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches);
/* host only: the box GAUSSIAN_BLUR runs three times along each axis for `radius` - what the blur kernel receives.  0, or -1 (radius not finite, negative
 * or above the cap; a NULL output) */
HIPDEC_API int hipdec_gaussian_box(double radius, int* r, uint32_t* ww, uint32_t* fw);

/* ---- recipe tensor output: affine steps inside augment chains - RandAugment / TrivialAugment / AutoAugment per sample, in one call ------------------------
 * RandAugment, TrivialAugment and AutoAugment draw, per sample, a few operations from ONE list of geometric (Rotate, ShearX/Y, TranslateX/Y) and colour
 * operations, in the sample's own order: one sample is [Rotate, Color], the next [Posterize, ShearX].  timm draws the warp filter per operation and fills
 * with the dataset mean.  The order changes the bytes - CONTRAST after a rotation takes its mean over the fill pixels, a blur after a shear smears the fill
 * edge - so the recipe stage is the augment stage with one more kind of step, not two stages in a row.  Bit-equal to Pillow, no tolerance.
 *
 * THE STAGE (hipdec_tensor_recipe).  As hipdec_tensor_augment, word for word - chains are hipdec_augment_chain, up to HIPDEC_AUGMENT_MAX_OPS steps, each on
 * the 8-bit result of the step before - with affines[0 .. n_affines - 1], the affine records of the call.  A step is one of:
 *  opcodes 1 .. 9       exactly the photo stage's definitions (hipdec_tensor_photo);
 *  opcodes 16, 17       exactly the augment stage's definitions (hipdec_tensor_augment);
 *  HIPDEC_RECIPE_AFFINE (value: an integer index i into affines)   PIL.Image.transform((w, h), AFFINE, affines[i].map, affines[i].filter,
 *    fillcolor = affines[i].fill) of the 8-bit result of the step before: exactly the arithmetic hipdec_tensor_warp states - BILINEAR, BICUBIC, and NEAREST on
 *    its table path (a1 == 0 && a3 == 0) or its fixed-point path - with src_width x src_height the sample's size (the stage does not resize) and an
 *    "outside" pixel holding the fill.  Several steps, of one entry or of many, may name the same record.
 * The last step of a chain writes the normalised tensor; if it is an affine step its fill is normalised as a pixel is (HIPDEC_FILL_COMPONENT).  There is
 * no element-domain fill inside a chain: an 8-bit intermediate cannot hold one.
 * Equalities: an empty chain gives hipdec_batch_to_tensor_oriented's bytes (decode-side forms); a chain without HIPDEC_RECIPE_AFFINE gives
 * hipdec_tensor_augment's bytes; a chain of one affine step gives hipdec_tensor_warp's bytes for that map, filter and a component fill; with a U8 / NHWC
 * output the stage chains with hipdec_tensor_warp, hipdec_tensor_photo, hipdec_tensor_augment and itself.
 *
 * THE DECODE-SIDE FORMS (hipdec_batch_to_tensor_recipe, hipdec_album_to_tensor_recipe): as the _augmented forms - sample e of the intermediate is what
 * hipdec_batch_to_tensor_oriented writes for entry e as U8 / NHWC of size src_width x src_height with desc->filter; a float dtype from a source above 8
 * bits is HIPDEC_ERR_UNSUPPORTED; the intermediate and the work memory come from the library's device pool and stay with the handle.
 *
 * Launches: the existing resize launch (decode-side forms); then per chain step at most ONE launch each of k_photo_hist, k_photo_apply, k_augment_hue,
 * k_augment_blur, k_recipe_affine_nearest, _bilinear and _bicubic, each over the compacted records of the entries whose operation at that step is of its
 * kind: at most 7 per step and 7 * HIPDEC_AUGMENT_MAX_OPS per call, whatever the number of entries.  The index tables of NEAREST scale-only maps (w + h
 * int32 each) travel behind the records in the same upload.  A step never reads the buffer it writes: the first step reads src_dev, the last writes
 * out_dev, the others alternate between two 8-bit intermediates.  Asynchronous on `stream`.  A recipe call counts in hipdec_recipe_stats only:
 * hipdec_warp_stats, hipdec_photo_stats and hipdec_augment_stats do not move.
 * Refused with HIPDEC_ERR_INVALID_ARGUMENT before anything is launched and before a device is touched, `out_dev` untouched, the entry and the operation
 * named: everything hipdec_tensor_augment refuses; n_affines < 0; and for HIPDEC_RECIPE_AFFINE a value that is not an integer 0 .. n_affines - 1, `affines`
 * NULL, a non-zero op.reserved, and of the record: a non-finite coefficient, |m[i]| >= 32000, a corner of [0, w] x [0, h] whose mapped coordinate has
 * magnitude >= 32000 (hipdec_tensor_warp's bounds), a filter other than NEAREST, BILINEAR, BICUBIC, a fill component outside 0 .. 255.  hipdec_tensor_photo
 * and hipdec_tensor_augment keep refusing opcode 32 as an unknown op.
 * Not part of it: perspective and quad maps inside a chain (hipdec_tensor_project is a stage of its own); a step that changes the size; a mask; element-domain fills; timm's SolarizeAdd and the *Increasing magnitude
 * schedules; samplers and magnitude tables (drawing stays with the caller); a clips entry point; staging source tiles in LDS. */
#define HIPDEC_RECIPE_AFFINE 32          /* value: integer index into the call's affines, 0 .. n_affines - 1 */
typedef struct hipdec_recipe_affine {
  hipdec_tensor_map map;       /* PIL's AFFINE data, as for hipdec_tensor_warp */
  int filter;                  /* HIPDEC_SCALE_NEAREST, _BILINEAR or _BICUBIC: per operation */
  int fill[3];                 /* Pillow's fillcolor: component values 0 .. 255 */
} hipdec_recipe_affine;        /* 64 bytes, no padding (the library asserts it) */
HIPDEC_API int hipdec_tensor_recipe(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_augment_chain* chains,
                                    const hipdec_recipe_affine* affines, int n_affines, const hipdec_tensor_desc* desc, int n, void* out_dev,
                                    size_t out_bytes, void* stream);
HIPDEC_API int hipdec_batch_to_tensor_recipe(hipdec_batch* b, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, const hipdec_recipe_affine* affines,
                                             int n_affines, int n_entries, void* out_dev, size_t out_bytes, void* stream);
HIPDEC_API int hipdec_album_to_tensor_recipe(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                             const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, const hipdec_recipe_affine* affines,
                                             int n_affines, int n_entries, void* out_dev, size_t out_bytes, void* stream);
/* counters since load: recipe calls that wrote anything, the entries they wrote, all kernel launches of the stage, and the affine steps among the
 * entries' steps (any may be NULL) */
HIPDEC_API void hipdec_recipe_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches, uint64_t* affine_steps);

/* counters since load: images through hipdec_image_transform, grid canvases handed out by hipdec_grid_read_plane_tracked (hipdec_image_scale counts in
 * hipdec_image_scale_stats) */
HIPDEC_API void hipdec_image_ops_stats(uint64_t* transforms, uint64_t* grid_canvases);
/* counters since load: conversions through hipdec_color_convert, input planes found device-resident, colour kernels launched */
HIPDEC_API void hipdec_color_boundary_stats(uint64_t* conversions, uint64_t* resident_planes, uint64_t* kernel_launches);
/* What the registry of handed-over planes holds right now: entries, and the device bytes they pin (every entry keeps its launch set's arena, a
 * transform result or a grid canvas alive; holders are counted once).  Bounded by age (HIPDEC_RESIDENT_TTL_MS, 3 s), by count, and by pinned bytes:
 * an eighth of the device's memory unless HIPDEC_RESIDENT_MAX_BYTES says otherwise (0: nothing is registered).  A device allocation that fails
 * empties the registry before its last retry. */
HIPDEC_API void hipdec_resident_plane_stats(uint64_t* entries, uint64_t* pinned_bytes);
/* Resident RGB: once a host has asked hipdec_color_convert() for interleaved RGB24 of 8-bit 4:2:0 planes in one op (what libheif's pipeline does
 * for heif_decode_image(.., heif_colorspace_RGB, heif_chroma_interleaved_RGB) through the integration op), the decoder's launch sets emit that RGB24
 * from the SAO kernel's store path (Op_YCbCr420_to_RGB24 / Op_YCbCr_to_RGB + Op_RGB_to_RGB24_32 fused, k_sao_rgb) and stage the rows to pinned host
 * memory beside the planes; a conversion whose planes are still the decoder's (every byte hashed) and whose colour description is the picture's VUI
 * is then a host copy.  Unfetched RGB spends the credit that requests earn, so a host that stops converting stops paying.  HIPDEC_NO_RESIDENT_RGB
 * switches it off.  images_produced: pictures decoded with RGB beside the planes; conversions_served: conversions answered from it. */
HIPDEC_API void hipdec_resident_rgb_stats(uint64_t* images_produced, uint64_t* conversions_served);

/* Op_to_hdr_planes (hdr_sdr.cc:25-109): 8-bit plane -> uint16 plane of out_bits (9..16): (v << (out_bits - 8)) | (v >> (16 - out_bits)). */
HIPDEC_API int hipdec_color_to_hdr(const void* in, size_t is, int w, int h, int out_bits, void* out, size_t os, void* stream);
/* Op_RRGGBBaa_swap_endianness (rgb2rgb.cc:647-764): interleaved RRGGBB (components 3) / RRGGBBAA (4) LE <-> BE. */
HIPDEC_API int hipdec_color_swap_endianness(const void* in, size_t is, int w, int h, int components, void* out, size_t os, void* stream);
/* PQ code values -> linear light (SMPTE ST 2084 / BT.2100 EOTF; 1.0 = 10000 cd/m2), float32 out with `components` values per pixel.
 * Input: 16-bit samples (interleaved RRGGBB[AA] rows or a plane, components = 1) of bit depth `bits`.  Not in the reference (libheif has
 * no transfer-function maths): BASELINE config 4's "PQ -> linear" stage; evaluated in fp64, tolerance against the published formula 1e-6 relative. */
HIPDEC_API int hipdec_color_pq_to_linear(const void* in, size_t is, int w, int h, int components, int bits, int big_endian, void* out, size_t os,
                                         void* stream);
/* The same for hybrid log-gamma code values (ARIB STD-B67 / BT.2100 HLG, transfer_characteristics 18): the inverse OETF per component, scene linear
 * light normalised to 1.0 (the display's OOTF is not applied).  Not in the reference either ("a real PQ / HLG EOTF stage"). */
HIPDEC_API int hipdec_color_hlg_to_linear(const void* in, size_t is, int w, int h, int components, int bits, int big_endian, void* out, size_t os,
                                          void* stream);
/* nclx.cc:143-173 get_YCbCr_to_RGB_coefficients: {r_cr, g_cb, g_cr, b_cb} */
HIPDEC_API void hipdec_color_coefficients(const hipdec_nclx* nclx, float out[4]);

#ifdef __cplusplus
}
#endif
#endif
