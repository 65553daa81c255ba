// decoder_album.inc — part of decoder.hip (one translation unit: the parts share its file-local types and helpers), included from there.
// Albums of grid photos on one device (hipdec_album_*).

// ---- albums of grid photos: one launch set, one fused paste ---------------------------------------------------------------
//
// hipdec_grid composes ONE photo per object: a host with K photos gets K launch sets, each bound by a single tile's CABAC critical path, and
// tiles x 3 strided copies per photo for the paste.  An album takes the tiles of K photos - every photo with its own grid geometry, tile size and
// output size - into ONE hipdec_batch, so rows x cols x K tiles' substreams fill the CABAC pool together, and pastes every tile plane of every photo
// into its canvas with ONE launch of k_album_paste (transform.hip: HeifPixelImage::copy_image_to, libheif/image/pixelimage.cc:1115-1172, over a
// job table in device memory).  The canvases - laid out as hipdec_grid's, 256-byte-aligned strides - share one arena allocation with the job table
// and feed the batch's colour, scaled and tensor stages through the same entry points and capture machinery, one launch each.
// Not here (include/heif_hipdec.h): sharding over devices, alpha / auxiliary images, the libheif hook, decoding straight into the canvas.
struct hipdec_album {
  struct Photo {
    int rows = 0, cols = 0, out_w = 0, out_h = 0, first_tile = 0, tile_w = 0, tile_h = 0;
    size_t off[3] = {0, 0, 0}, stride[3] = {0, 0, 0};   // of the canvas planes inside `canvas`
  };
  std::vector<Photo> photos;
  std::unique_ptr<hipdec_batch> batch;   // all tiles of all photos; owned
  int device = 0, bits = 8, chroma_format_idc = 1;
  int csw = 2, csh = 2;                  // chroma subsampling of the tiles (and of the canvases)
  uint8_t* canvas = nullptr;             // the canvases of all photos, then the job table
  size_t canvas_capacity = 0;
  const PasteJob* jobs_dev = nullptr;
  int n_jobs = 0;
  uint32_t max_rows = 0;                 // of any job: sizes the launch
  hipEvent_t paste_ev[2] = {nullptr, nullptr};   // around the paste launch of the last run
  ColorBatchState color, color_scaled, color_tensor;   // parameter blocks of the three output stages (their own, as hipdec_batch's)
  ColorBatchState color_oriented;                      // ... and of the oriented forms
  ColorBatchState color_margin;                        // ... and the margin blocks of hipdec_album_to_tensor_placed
  ColorBatchState color_packed;                        // ... and of hipdec_album_to_tensor_packed
  uint64_t max_pixels = 0;
  bool ran = false;
  ~hipdec_album()
  {
    DeviceScope scope(device);
    batch.reset();   // waits for everything enqueued for the album: every stage marks the batch's `done`
    for (hipEvent_t e : paste_ev) if (e) (void)hipEventDestroy(e);
    color_batch_state_free(color);
    color_batch_state_free(color_scaled);
    color_batch_state_free(color_tensor);
    color_batch_state_free(color_oriented);
    color_batch_state_free(color_margin);
    color_batch_state_free(color_packed);
    if (canvas) arena_release(canvas, canvas_capacity);
  }
};

namespace {

std::atomic<uint64_t> g_album_albums{0}, g_album_photos{0}, g_album_pastes{0};

// the canvas of photo p as the picture the colour entry points convert (VUI colour description: the photo's tile 0, as hipdec_grid_to_rgb)
RgbSource album_source(const hipdec_album* a, int p)
{
  const hipdec_album::Photo& ph = a->photos[(size_t)p];
  return RgbSource{{a->canvas + ph.off[0], a->canvas + ph.off[1], a->canvas + ph.off[2]}, {ph.stride[0], ph.stride[1], ph.stride[2]},
                   ph.out_w, ph.out_h, a->chroma_format_idc, a->bits > 8, &a->batch->pics[(size_t)ph.first_tile].info, a->max_pixels};
}

int album_rgb_entries(const char* who, hipdec_album* a, int out_chroma, const int* orientations, bool oriented, const int* out_widths, const int* out_heights, int filter,
                      void* const* outs_dev, const size_t* out_strides, void* stream);   // (below)

}  // namespace

extern "C" {

int hipdec_album_create(hipdec_album** out, int n_photos, const hipdec_album_photo* photos, const void* const* tile_data, const size_t* tile_sizes,
                        int n_tiles, uint64_t max_image_size_pixels)
{
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: NULL out");
  *out = nullptr;
  if (!photos || !tile_data || !tile_sizes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: NULL photos, tile_data or tile_sizes");
  if (n_photos <= 0 || n_tiles <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: %d photos of %d tiles", n_photos, n_tiles);
  return guarded("album_create", [&]() -> int {
    // what the arguments alone decide
    std::vector<std::pair<int64_t, int>> ranges;   // (first tile, photo)
    for (int p = 0; p < n_photos; p++) {
      const hipdec_album_photo& q = photos[p];
      if (q.reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: photo %d: reserved must be 0", p);
      if (q.rows <= 0 || q.cols <= 0 || q.rows > 256 || q.cols > 256)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: photo %d: a grid of %d x %d tiles (1 .. 256 each way)", p, q.rows, q.cols);
      if (q.out_width <= 0 || q.out_height <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: photo %d: output size %d x %d", p, q.out_width, q.out_height);
      if (q.first_tile < 0 || (int64_t)q.first_tile + (int64_t)q.rows * q.cols > (int64_t)n_tiles)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: photo %d: tiles %d .. %lld lie outside the %d tiles given", p, q.first_tile,
                         (long long)q.first_tile + (long long)q.rows * q.cols - 1, n_tiles);
      if (max_image_size_pixels && (uint64_t)q.out_width * (uint64_t)q.out_height > max_image_size_pixels)
        return set_error(HIPDEC_ERR_LIMIT, "album_create: photo %d: output of %d x %d pixels exceeds max_image_size_pixels", p, q.out_width, q.out_height);
      ranges.emplace_back((int64_t)q.first_tile, p);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); k++) {
      const hipdec_album_photo& prev = photos[ranges[k - 1].second];
      if (ranges[k].first < ranges[k - 1].first + (int64_t)prev.rows * prev.cols)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_create: photos %d and %d share tiles", ranges[k - 1].second, ranges[k].second);
    }
    if (int rc = ensure_init()) return rc;
    std::unique_ptr<hipdec_album> a(new hipdec_album());
    a->device = active_device();
    a->max_pixels = max_image_size_pixels;
    a->photos.resize((size_t)n_photos);
    // what the tiles' headers decide: hipdec_grid_create's rules per photo, one chroma format and one bit depth per album - before anything is allocated
    const std::function<int(const hipdec_batch&)> geometry = [&](const hipdec_batch& b) -> int {
      const hipdec_image_info& I0 = b.pics[(size_t)photos[0].first_tile].info;
      a->bits = I0.bit_depth_luma; a->chroma_format_idc = I0.chroma_format_idc;
      a->csw = (I0.chroma_format_idc == 1 || I0.chroma_format_idc == 2) ? 2 : 1;
      a->csh = I0.chroma_format_idc == 1 ? 2 : 1;
      for (int p = 0; p < n_photos; p++) {
        const hipdec_album_photo& q = photos[p];
        hipdec_album::Photo& ph = a->photos[(size_t)p];
        const hipdec_image_info& T0 = b.pics[(size_t)q.first_tile].info;
        ph.rows = q.rows; ph.cols = q.cols; ph.out_w = q.out_width; ph.out_h = q.out_height; ph.first_tile = q.first_tile;
        ph.tile_w = T0.width; ph.tile_h = T0.height;
        for (int t = 0; t < q.rows * q.cols; t++) {
          const hipdec_image_info& T = b.pics[(size_t)(q.first_tile + t)].info;
          if (T.width != ph.tile_w || T.height != ph.tile_h) return set_error(HIPDEC_ERR_BITSTREAM, "album_create: photo %d: tiles differ in size", p);
          if (T.bit_depth_luma != a->bits || T.chroma_format_idc != a->chroma_format_idc)
            return set_error(HIPDEC_ERR_BITSTREAM, "album_create: photo %d: tile %d differs from the album's bit depth or chroma format", p, t);
        }
        if (q.out_width > q.cols * ph.tile_w || q.out_height > q.rows * ph.tile_h)
          return set_error(HIPDEC_ERR_BITSTREAM, "album_create: photo %d: the output size exceeds the tiled area", p);
        if (a->chroma_format_idc && ((ph.tile_w % a->csw) || (ph.tile_h % a->csh)))
          return set_error(HIPDEC_ERR_UNSUPPORTED, "album_create: photo %d: subsampled tiles with odd dimensions", p);
      }
      return 0;
    };
    a->batch.reset(new hipdec_batch());
    if (int rc = build_batch(*a->batch, n_tiles, tile_data, tile_sizes, max_image_size_pixels, nullptr, nullptr, nullptr, &geometry)) return rc;
    const hipdec_batch& b = *a->batch;
    // the canvases, each laid out as hipdec_grid's, and the job table behind them
    const size_t es = a->bits > 8 ? 2 : 1;
    const int ncomp = a->chroma_format_idc ? 3 : 1;
    size_t o = 0;
    for (hipdec_album::Photo& ph : a->photos) {
      const size_t cw = a->chroma_format_idc ? ((size_t)ph.out_w + a->csw - 1) / a->csw : 0, ch = a->chroma_format_idc ? ((size_t)ph.out_h + a->csh - 1) / a->csh : 0;
      ph.stride[0] = ((size_t)ph.out_w * es + 255) & ~(size_t)255; ph.off[0] = o; o += ph.stride[0] * (size_t)ph.out_h;
      ph.stride[1] = ph.stride[2] = (cw * es + 255) & ~(size_t)255;
      ph.off[1] = o; o += ph.stride[1] * ch; ph.off[2] = o; o += ph.stride[2] * ch;
    }
    const size_t off_jobs = o;
    HIPDEC_CHECK_HIP(arena_acquire((void**)&a->canvas, off_jobs + (size_t)n_tiles * 3 * sizeof(PasteJob) + 256, &a->canvas_capacity));
    std::vector<PasteJob> jobs;
    for (const hipdec_album::Photo& ph : a->photos)
      for (int t = 0; t < ph.rows * ph.cols; t++) {
        const int x0 = (t % ph.cols) * ph.tile_w, y0 = (t / ph.cols) * ph.tile_h;
        const int w = std::min(ph.tile_w, ph.out_w - x0), h = std::min(ph.tile_h, ph.out_h - y0);   // clipped to the output (pixelimage.cc:1130-1160)
        if (w <= 0 || h <= 0) continue;
        const PicParams& P = b.params[(size_t)(ph.first_tile + t)];
        for (int c = 0; c < ncomp; c++) {
          const size_t sw = c ? (size_t)a->csw : 1, sh = c ? (size_t)a->csh : 1;
          const size_t pw = ((size_t)w + sw - 1) / sw, rows = ((size_t)h + sh - 1) / sh;
          const size_t px = (size_t)x0 / sw, py = (size_t)y0 / sh;
          PasteJob j;
          j.src = b.arena + P.off_out[c]; j.src_stride = P.out_stride[c];
          j.dst = a->canvas + ph.off[c] + py * ph.stride[c] + px * es; j.dst_stride = ph.stride[c];
          j.width_bytes = (uint32_t)(pw * es); j.rows = (uint32_t)rows;
          a->max_rows = std::max(a->max_rows, j.rows);
          jobs.push_back(j);
        }
      }
    a->n_jobs = (int)jobs.size();
    a->jobs_dev = (const PasteJob*)(a->canvas + off_jobs);
    HIPDEC_CHECK_HIP(hipMemcpy(a->canvas + off_jobs, jobs.data(), jobs.size() * sizeof(PasteJob), hipMemcpyHostToDevice));
    for (hipEvent_t& e : a->paste_ev) HIPDEC_CHECK_HIP(hipEventCreate(&e));
    g_album_albums++; g_album_photos += (uint64_t)n_photos;
    *out = a.release();
    return 0;
  });
}

void hipdec_album_free(hipdec_album* a) { delete a; }
int hipdec_album_count(const hipdec_album* a) { return a ? (int)a->photos.size() : set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_count: NULL album"); }

int hipdec_album_info(const hipdec_album* a, int photo, hipdec_image_info* info)
{
  if (!a || !info || photo < 0 || photo >= (int)a->photos.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_info: bad arguments");
  const hipdec_album::Photo& ph = a->photos[(size_t)photo];
  *info = a->batch->pics[(size_t)ph.first_tile].info;
  info->width = ph.out_w; info->height = ph.out_h;
  info->chroma_width = a->chroma_format_idc ? (ph.out_w + a->csw - 1) / a->csw : 0; info->chroma_height = a->chroma_format_idc ? (ph.out_h + a->csh - 1) / a->csh : 0;
  info->coded_width = ph.cols * ph.tile_w; info->coded_height = ph.rows * ph.tile_h;
  size_t bytes = 0; int subs = 0;
  for (int t = 0; t < ph.rows * ph.cols; t++) { const hipdec_image_info& T = a->batch->pics[(size_t)(ph.first_tile + t)].info; bytes += T.bitstream_bytes; subs += T.num_substreams; }
  info->bitstream_bytes = bytes; info->num_substreams = subs;
  return 0;
}

int hipdec_album_run(hipdec_album* a, void* stream)
{
  if (!a) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_run: NULL album");
  DeviceScope scope(a->device);
  return guarded("album_run", [&]() -> int {
    hipdec_batch* b = a->batch.get();
    if (int rc = hipdec_batch_run(b, stream)) return rc;
    hipStream_t s = follow_stream(b, stream);   // with stage overlap the pixel stages run on the post stream: the paste waits for them
    HIPDEC_CHECK_HIP(hipEventRecord(a->paste_ev[0], s));
    const int rc = album_paste_launch(a->jobs_dev, a->n_jobs, a->max_rows, s);
    HIPDEC_CHECK_HIP(hipEventRecord(a->paste_ev[1], s));
    b->mark_done(s);
    if (rc) return rc;
    a->ran = true;
    g_album_pastes++;
    return 0;
  });
}

int hipdec_album_status(hipdec_album* a)
{
  if (!a || !a->ran) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_status: album has not been run");
  return hipdec_batch_status(a->batch.get());   // (waits for the paste and the output stages too: each of them marked the batch's `done`)
}

int hipdec_album_paste_timing_us(hipdec_album* a, float* us)
{
  if (!a || !a->ran || !us) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_paste_timing: album has not been run");
  DeviceScope scope(a->device);
  float ms = 0;
  HIPDEC_CHECK_HIP(hipEventSynchronize(a->paste_ev[1]));
  HIPDEC_CHECK_HIP(hipEventElapsedTime(&ms, a->paste_ev[0], a->paste_ev[1]));
  *us = ms * 1000.0f;
  return 0;
}

int hipdec_album_canvas_plane(hipdec_album* a, int photo, int c, const void** dptr, size_t* stride)
{
  if (!a || photo < 0 || photo >= (int)a->photos.size() || c < 0 || c > 2 || !dptr || !stride) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_canvas_plane: bad arguments");
  if (c > 0 && !a->chroma_format_idc) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_canvas_plane: monochrome album has no chroma planes");
  const hipdec_album::Photo& ph = a->photos[(size_t)photo];
  *dptr = a->canvas + ph.off[c]; *stride = ph.stride[c];
  return 0;
}

int hipdec_album_read_plane(hipdec_album* a, int photo, int c, void* dst_host, size_t dst_stride)
{
  if (!a || !a->ran || photo < 0 || photo >= (int)a->photos.size() || c < 0 || c > 2 || !dst_host) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_read_plane: bad arguments");
  if (c > 0 && !a->chroma_format_idc) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_read_plane: monochrome album has no chroma planes");
  if (int rc = hipdec_album_status(a)) return rc;
  DeviceScope scope(a->device);
  const hipdec_album::Photo& ph = a->photos[(size_t)photo];
  const size_t es = a->bits > 8 ? 2 : 1;
  const size_t sw = c ? (size_t)a->csw : 1, sh = c ? (size_t)a->csh : 1;
  const size_t w = ((size_t)ph.out_w + sw - 1) / sw, h = ((size_t)ph.out_h + sh - 1) / sh;
  if (dst_stride < w * es) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_read_plane: dst_stride %zu is smaller than a row of %zu bytes", dst_stride, w * es);
  return copy_rows_to_host(dst_host, dst_stride, a->canvas + ph.off[c], ph.stride[c], w * es, (int)h, default_stream());
}

// hipdec_batch_to_rgb_all over the canvases: every photo through the planner rules of hipdec_batch_to_rgb in capture mode, then ONE launch
int hipdec_album_to_rgb_all(hipdec_album* a, int out_chroma, void* const* outs_dev, const size_t* out_strides, void* stream)
{
  if (!a || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_rgb_all: bad arguments");
  DeviceScope scope(a->device);
  hipdec_batch* b = a->batch.get();
  hipStream_t s = follow_stream(b, stream);
  color_capture_begin();
  for (int p = 0; p < (int)a->photos.size(); p++) {
    int rc = outs_dev[p] ? 0 : set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb: bad arguments");
    if (!rc) rc = source_to_rgb(album_source(a, p), out_chroma, outs_dev[p], out_strides[p], nullptr, [&]() -> void* { return (void*)s; });
    if (rc) { color_capture_abort(); return rc; }
  }
  const int rc = color_capture_launch(a->color, s);
  b->mark_done(s);
  return rc;
}

// hipdec_batch_to_rgb_scaled_all over the canvases
int hipdec_album_to_rgb_scaled_all(hipdec_album* a, int out_chroma, const int* out_widths, const int* out_heights, int filter, void* const* outs_dev,
                                   const size_t* out_strides, void* stream)
{
  if (resample_filter(filter)) {   // bilinear / bicubic: the photos as U8 / NHWC entries of ONE k_resample launch, as the oriented form records them
    if (out_chroma != 10) return set_error(HIPDEC_ERR_UNSUPPORTED, "album_to_rgb_scaled_all: out_chroma %d with filter %d (bilinear / bicubic write interleaved RGB24, out_chroma 10)", out_chroma, filter);
    return album_rgb_entries("album_to_rgb_scaled_all", a, out_chroma, nullptr, false, out_widths, out_heights, filter, outs_dev, out_strides, stream);
  }
  if (!a || !out_widths || !out_heights || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_rgb_scaled_all: bad arguments");
  DeviceScope scope(a->device);
  hipdec_batch* b = a->batch.get();
  hipStream_t s = follow_stream(b, stream);
  color_capture_begin();
  for (int p = 0; p < (int)a->photos.size(); p++) {
    const ScaleRequest rq{out_widths[p], out_heights[p], filter};
    int rc = outs_dev[p] ? 0 : set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_rgb: bad arguments");
    if (!rc) rc = source_to_rgb(album_source(a, p), out_chroma, outs_dev[p], out_strides[p], &rq, [&]() -> void* { return (void*)s; });
    if (rc) { color_capture_abort(); return rc; }
  }
  const int rc = color_capture_launch_scaled(a->color_scaled, filter, s);
  b->mark_done(s);
  return rc;
}

}  // extern "C"

namespace {
// hipdec_batch_to_rgb_scaled_oriented_all over the canvases; oriented false: the unoriented call with a resampling filter (no code, not counted as oriented)
int album_rgb_entries(const char* who, hipdec_album* a, int out_chroma, const int* orientations, bool oriented, const int* out_widths, const int* out_heights, int filter,
                      void* const* outs_dev, const size_t* out_strides, void* stream)
{
  if (!a || !out_widths || !out_heights || !outs_dev || !out_strides) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  const int n = (int)a->photos.size();
  for (int p = 0; p < n; p++) {
    if (!outs_dev[p]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: photo %d: no output", who, p);
    if (int rc = rgb_oriented_check_item(who, p, out_chroma, orientations ? orientations[p] : 0, out_widths[p], out_heights[p], filter, out_strides[p])) return rc;
  }
  DeviceScope scope(a->device);
  return guarded(who, [&]() -> int {
    hipdec_batch* b = a->batch.get();
    hipStream_t s = follow_stream(b, stream);
    color_tensor_begin();
    for (int p = 0; p < n; p++)
      if (int rc = rgb_oriented_record(who, album_source(a, p), oriented ? (orientations ? orientations[p] : 0) : -1, out_widths[p], out_heights[p], filter, outs_dev[p], out_strides[p])) {
        color_tensor_abort();
        return rc;
      }
    const int rc = color_tensor_launch(a->color_oriented, filter, HIPDEC_TENSOR_U8, s);
    b->mark_done(s);
    return rc;
  });
}

// hipdec_batch_to_tensor over the canvases: entry.item names a photo, the window lies in its output size; oriented and placed (pa): as batch_to_tensor_impl
int album_to_tensor_impl(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations, bool oriented, int n_entries,
                         void* out_dev, size_t out_bytes, void* stream, const PlacedArgs* pa = nullptr, const PackedSpec* ps = nullptr)
{
  if (!a || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_tensor: bad arguments");
  size_t bytes = 0;
  hipdec_tensor_desc unit;
  PackedArgs pk{nullptr, 0, 1};
  if (ps) if (int rc = packed_check_desc("album_to_tensor_packed", desc, &unit)) return rc;
  const bool composed = pa && pa->composed;
  ComposePlan plan;
  if (composed && n_entries < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_tensor_composed: %d entries", n_entries);
  if (int rc = tensor_check_desc("album_to_tensor", ps ? &unit : desc, composed ? pa->n_canvases : n_entries, &bytes)) return rc;
  if (oriented) if (int rc = check_orientations("album_to_tensor_oriented", "entry", orientations, n_entries)) return rc;
  const bool framed = pa && pa->framed && pa->places;
  if (composed) { if (int rc = composed_check("album_to_tensor_composed", desc, *pa, n_entries, &plan)) return rc; }
  else if (pa) if (int rc = placed_check(pa->framed ? "album_to_tensor_framed" : "album_to_tensor_placed", desc, *pa, n_entries)) return rc;
  if (ps) { if (int rc = packed_check("album_to_tensor_packed", desc, ps->samples, ps->patches, n_entries, out_bytes, &pk)) return rc; }
  else if (out_bytes < bytes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_tensor: out_bytes %zu is smaller than the tensor of %zu bytes", out_bytes, bytes);
  // (everything above is decided without reading the handle)
  const int n_photos = (int)a->photos.size();
  if (!entries && n_entries != n_photos)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_tensor: %d entries without an entry list, the album has %d photos", n_entries, n_photos);
  DeviceScope scope(a->device);
  if (!ps && a->max_pixels && (uint64_t)desc->width * (uint64_t)desc->height > a->max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "album_to_tensor: output of %d x %d pixels exceeds max_image_size_pixels", desc->width, desc->height);
  for (int e = 0; ps && a->max_pixels && e < n_entries; e++)
    if ((uint64_t)pk.samples[e].width * (uint64_t)pk.samples[e].height > a->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "album_to_tensor_packed: entry %d: sample of %d x %d pixels exceeds max_image_size_pixels", e, pk.samples[e].width, pk.samples[e].height);
  for (int e = 0; framed && a->max_pixels && e < n_entries; e++)
    if ((uint64_t)pa->places[e].width * (uint64_t)pa->places[e].height > a->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "album_to_tensor_framed: entry %d: rectangle of %d x %d pixels exceeds max_image_size_pixels", e, pa->places[e].width, pa->places[e].height);
  for (int e = 0; composed && a->max_pixels && e < n_entries; e++)
    if ((uint64_t)pa->tiles[e].place.width * (uint64_t)pa->tiles[e].place.height > a->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "album_to_tensor_composed: entry %d: rectangle of %d x %d pixels exceeds max_image_size_pixels", e, pa->tiles[e].place.width,
                       pa->tiles[e].place.height);
  return guarded("album_to_tensor", [&]() -> int {
    hipdec_batch* b = a->batch.get();
    hipStream_t s = follow_stream(b, stream);
    const size_t entry_bytes = bytes / (size_t)(composed ? pa->n_canvases : n_entries);
    std::vector<CanvasMargin> margins(pa && !composed ? (size_t)n_entries : 0);
    color_tensor_begin();
    for (int e = 0; e < n_entries; e++) {
      const int p = entries ? entries[e].item : e;
      if (p < 0 || p >= n_photos) { color_tensor_abort(); return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "album_to_tensor: entry %d names photo %d of %d", e, p, n_photos); }
      const RgbSource S = album_source(a, p);
      const hipdec_image_info& I = *S.info;
      int left, top, rw, rh;
      int rc = tensor_window("album_to_tensor", entries ? entries + e : nullptr, e, S.width, S.height, &left, &top, &rw, &rh);
      hipdec_nclx nclx{1, I.colour_primaries, I.transfer_characteristics, I.matrix_coeffs, I.full_range_flag};
      hipdec_tensor_desc sample = *desc;
      void* elem0 = (uint8_t*)out_dev + (size_t)e * entry_bytes;
      size_t pitch = 0;
      int plane_rows = 0;
      int vis[4];
      if (pa) {
        if (!rc) rc = placed_check_component(composed ? "album_to_tensor_composed" : (pa->framed ? "album_to_tensor_framed" : "album_to_tensor_placed"), desc, *pa, e,
                                             S.wide ? I.bit_depth_luma : 8);
        if (composed) composed_entry(desc, *pa, e, out_dev, entry_bytes, &sample, &elem0);
        else placed_entry(desc, *pa, e, out_dev, entry_bytes, &sample, &elem0, &margins[(size_t)e], vis);
        pitch = (size_t)desc->width * (desc->layout == HIPDEC_TENSOR_NHWC ? 3 : 1); plane_rows = desc->height;
      }
      if (ps) packed_entry(desc, pk, e, out_dev, &sample, &elem0);
      const size_t n_req = composed ? plan.pieces[(size_t)e].size() : 1;   // (as batch_to_tensor_impl: a composed entry records one request per piece)
      if (!rc && composed) rc = tensor_check_resample_depth("album_to_tensor_composed", desc, S.wide ? I.bit_depth_luma : 8);
      for (size_t q = 0; !rc && q < n_req; q++) {
        if (composed) compose_piece_window(plan.pieces[(size_t)e][q], pa->tiles[e].place, vis);
        rc = tensor_record_entry("album_to_tensor", S.plane[0], S.stride[0], S.plane[1], S.stride[1], S.plane[2], S.stride[2], S.width, S.height,
                                 S.wide ? I.bit_depth_luma : 8, S.chroma_format_idc, &nclx, &nclx, &sample, left, top, rw, rh, entries ? entries[e].flip : 0,
                                 elem0, oriented ? (orientations ? orientations[e] : 0) : -1, pitch, plane_rows, pk.patch, pk.merge, 1, nullptr,
                                 framed || composed ? vis : nullptr, composed);
      }
      if (rc) { color_tensor_abort(); return rc; }
    }
    int rc = color_tensor_launch(ps ? a->color_packed : (oriented || resample_filter(desc->filter) ? a->color_oriented : a->color_tensor), desc->filter, desc->dtype, s);
    if (!rc && composed) rc = composed_cover(a->color_margin, desc, *pa, plan, out_dev, entry_bytes, s);
    else if (!rc && pa) rc = canvas_margin_launch(a->color_margin, margins.data(), n_entries, desc->dtype, s);
    b->mark_done(s);
    if (!rc && pa && !pa->framed && !composed) placed_note_call((uint64_t)n_entries);
    if (!rc && pa && pa->framed) framed_note_call((uint64_t)n_entries);
    if (!rc && composed) composed_note_call((uint64_t)n_entries, plan.n_pieces, plan.hidden);
    if (!rc && ps) packed_note_call((uint64_t)n_entries, pk.patch > 0);
    return rc;
  });
}

// the album forms of batch_to_tensor_two_stage: the stage's tables, intermediate and work memory are those of the album's batch
template <typename Stage>
int album_to_tensor_two_stage(const char* who, hipdec_album* a, const Stage& stage, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                              int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return to_tensor_two_stage(
      who, a, stage, desc, entries, orientations, n_entries, out_dev, out_bytes, stream,
      [&]() { return TwoStageSource{a->batch.get(), a->device, (int)a->photos.size(), false, a->max_pixels}; },
      [&](int p) { const RgbSource S = album_source(a, p); return S.wide ? S.info->bit_depth_luma : 8; },
      [&](const hipdec_tensor_desc* mid, void* out, size_t bytes, void* st) { return album_to_tensor_impl(a, mid, entries, orientations, true, n_entries, out, bytes, st); });
}
}  // namespace

extern "C" {

int hipdec_album_to_tensor(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, int n_entries, void* out_dev, size_t out_bytes,
                           void* stream)
{
  return album_to_tensor_impl(a, desc, entries, nullptr, false, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_oriented(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations, int n_entries,
                                    void* out_dev, size_t out_bytes, void* stream)
{
  return album_to_tensor_impl(a, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_placed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev, size_t out_bytes,
                                  void* stream)
{
  const PlacedArgs pa{places, fill, mask_dev};
  return album_to_tensor_impl(a, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_album_to_tensor_framed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_place* places, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, void* out_dev, size_t out_bytes,
                                  void* stream)
{
  const PlacedArgs pa{places, fill, mask_dev, true};
  return album_to_tensor_impl(a, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_album_to_tensor_composed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                    const hipdec_tensor_tile* tiles, const hipdec_tensor_fill* fill, void* mask_dev, int n_entries, int n_canvases, void* out_dev,
                                    size_t out_bytes, void* stream)
{
  const PlacedArgs pa{nullptr, fill, mask_dev, false, true, tiles, n_canvases};
  return album_to_tensor_impl(a, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, &pa);
}

int hipdec_album_to_tensor_packed(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  const PackedSpec ps{samples, patches};
  return album_to_tensor_impl(a, desc, entries, orientations, true, n_entries, out_dev, out_bytes, stream, nullptr, &ps);
}

int hipdec_album_to_tensor_warped(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_warp_desc* warp, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, int n_entries, void* out_dev,
                                  size_t out_bytes, void* stream)
{
  return album_to_tensor_two_stage("album_to_tensor_warped", a, WarpStage{warp, maps, fill}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_projected(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                     const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill, int n_entries, void* out_dev,
                                     size_t out_bytes, void* stream)
{
  return album_to_tensor_two_stage("album_to_tensor_projected", a, ProjectStage{warp, maps, fill}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_photo(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                 const hipdec_photo_desc* photo, const hipdec_photo_chain* chains, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return album_to_tensor_two_stage("album_to_tensor_photo", a, PhotoStage{photo, chain_view(chains)}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_augmented(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                     const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return album_to_tensor_two_stage("album_to_tensor_augmented", a, PhotoStage{photo, chain_view(chains)}, desc, entries, orientations, n_entries, out_dev, out_bytes, stream);
}

int hipdec_album_to_tensor_recipe(hipdec_album* a, const hipdec_tensor_desc* desc, const hipdec_tensor_entry* entries, const int* orientations,
                                  const hipdec_photo_desc* photo, const hipdec_augment_chain* chains, const hipdec_recipe_affine* affines, int n_affines,
                                  int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return album_to_tensor_two_stage("album_to_tensor_recipe", a, PhotoStage{photo, recipe_view(chains, affines, n_affines)}, desc, entries, orientations, n_entries,
                                   out_dev, out_bytes, stream);
}

int hipdec_album_to_rgb_scaled_oriented_all(hipdec_album* a, int out_chroma, const int* orientations, const int* out_widths, const int* out_heights, int filter,
                                            void* const* outs_dev, const size_t* out_strides, void* stream)
{
  return album_rgb_entries("album_to_rgb_scaled_oriented_all", a, out_chroma, orientations, true, out_widths, out_heights, filter, outs_dev, out_strides, stream);
}

void hipdec_album_stats(uint64_t* albums, uint64_t* photos, uint64_t* paste_launches)
{
  if (albums) *albums = g_album_albums.load();
  if (photos) *photos = g_album_photos.load();
  if (paste_launches) *paste_launches = g_album_pastes.load();
}

}  // extern "C"
