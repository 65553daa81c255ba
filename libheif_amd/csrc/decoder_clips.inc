// decoder_clips.inc — part of decoder.hip (one translation unit: the parts share its file-local types and helpers), included from there.
// Clips (hipdec_clips_*): the samples of several sequence tracks as ONE launch set whose pictures stay in device memory, and video tensors from them.

// ---- clips ---------------------------------------------------------------------------------------------------------------------------------
// run_chain_set (decoder_chains.inc) builds one hipdec_batch from the queued samples of the decoder objects that asked within a few milliseconds of
// each other; a clips object builds the same batch - build_batch with a ChainPlan, every track from a fresh SeqContext - from samples the host hands
// over at once, and keeps it.  Its frames are the tracks' pictures in OUTPUT order; the tensor stage of the batch (tensor_record_entry, the recorded
// blocks of color.hip) serves them with the strides of a video tensor: a frame of an N x C x T x H x W clip is an oriented entry whose channel planes
// are T * H rows apart, a frame of a token sequence with a temporal patch a patch entry whose tokens hold Tp frames.
struct hipdec_clips {
  struct Frame { int item = 0, sample = 0, poc = 0, sequence = 0; };
  std::vector<std::vector<Frame>> frames;   // per track, in output order
  std::unique_ptr<hipdec_batch> batch;      // the launch set; handed out borrowed (hipdec_clips_batch)
  int device = 0;
  ~hipdec_clips()
  {
    DeviceScope scope(device);
    batch.reset();   // waits for everything enqueued for it
  }
};

namespace {

std::atomic<uint64_t> g_clips_sets{0}, g_clips_tracks{0}, g_clips_frames{0}, g_clips_tensor_calls{0};

// dev knob, read once: box entries with folded code 0 / 4 go through k_oriented_box as the other codes do (tools/measure_clip_output.py compares the routes)
bool clips_no_strided_box()
{
  static const bool off = getenv("HIPDEC_CLIP_NO_STRIDED_BOX") != nullptr;
  return off;
}

// what the clip description alone decides; *Tp: frames per token (1 for dense clips)
int clip_check_desc(const char* who, const hipdec_clip_desc* clip, const hipdec_tensor_desc* desc, const hipdec_tensor_patches* patches, bool packed, int* Tp)
{
  if (!clip) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: no clip description", who);
  if (clip->frames < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: %d frames per clip", who, clip->frames);
  if (clip->reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: clip.reserved is %d, not 0", who, clip->reserved);
  if (clip->order != HIPDEC_CLIP_FRAME_MAJOR && clip->order != HIPDEC_CLIP_CHANNEL_MAJOR) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown clip order %d", who, clip->order);
  const int patch = packed && patches ? patches->patch : 0;
  if (clip->temporal_patch < 0 || clip->temporal_patch > 16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: temporal_patch %d is not 0 .. 16", who, clip->temporal_patch);
  if (!patch && clip->temporal_patch > 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: temporal_patch %d without patches (dense clips take 0 or 1)", who, clip->temporal_patch);
  *Tp = clip->temporal_patch > 1 ? clip->temporal_patch : 1;
  if (clip->frames % *Tp) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: %d frames per clip are not a multiple of temporal_patch %d", who, clip->frames, *Tp);
  if (patch && clip->order != HIPDEC_CLIP_FRAME_MAJOR) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: channel-major order with patches (token sequences are frame-major)", who);
  if (desc && clip->order == HIPDEC_CLIP_CHANNEL_MAJOR && desc->layout == HIPDEC_TENSOR_NHWC)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: channel-major order with HIPDEC_TENSOR_NHWC (N C T H W is the channel-major layout)", who);
  return 0;
}

// the packed call's checks of the per-clip sizes and element ranges (packed_check, with 3 * T * w * h elements per entry)
int clip_packed_check(const char* who, const hipdec_tensor_desc* d, const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int T, int n_entries, size_t out_bytes,
                      PackedArgs* pk)
{
  if (!samples) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: no samples", who);
  if (int rc = packed_check_patches(who, patches)) return rc;
  pk->samples = samples; pk->patch = patches ? patches->patch : 0; pk->merge = patches ? patches->merge : 1;
  const uint64_t room = (uint64_t)out_bytes / tensor_elem_bytes(d->dtype);
  std::vector<std::pair<uint64_t, int>> order((size_t)n_entries);
  auto len_of = [&](const hipdec_tensor_sample& sm) { return 3ull * (uint64_t)T * (uint64_t)sm.width * (uint64_t)sm.height; };
  for (int e = 0; e < n_entries; e++) {
    const hipdec_tensor_sample& sm = samples[e];
    if (int rc = packed_check_size(who, e, sm.width, sm.height, pk->patch, pk->merge)) return rc;
    if ((uint64_t)sm.width * (uint64_t)sm.height > ((1ull << 62) / 3ull) / (uint64_t)T) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: clip too large", who, e);
    const uint64_t len = len_of(sm);
    if (sm.offset > room || len > room - sm.offset)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: clip of %llu elements at offset %llu leaves the output of %llu elements", who, e,
                       (unsigned long long)len, (unsigned long long)sm.offset, (unsigned long long)room);
    order[(size_t)e] = std::make_pair(sm.offset, e);
  }
  std::sort(order.begin(), order.end());
  for (int k = 0; k + 1 < n_entries; k++) {
    const hipdec_tensor_sample& a = samples[order[(size_t)k].second];
    if (a.offset + len_of(a) > order[(size_t)k + 1].first)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: its elements overlap those of entry %d", who, order[(size_t)k + 1].second, order[(size_t)k].second);
  }
  return 0;
}

// hipdec_clips_to_tensor and - with ps - hipdec_clips_to_tensor_packed: batch_to_tensor_impl's checks, windows and planner rules, T recorded blocks per entry
int clips_to_tensor_impl(hipdec_clips* c, const hipdec_tensor_desc* desc, const hipdec_clip_desc* clip, const hipdec_tensor_entry* entries, const int* frames,
                         const int* orientations, int n_entries, void* out_dev, size_t out_bytes, void* stream, const PackedSpec* ps)
{
  const char* who = ps ? "clips_to_tensor_packed" : "clips_to_tensor";
  if (!c || !out_dev || !entries) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  size_t bytes = 0;
  hipdec_tensor_desc unit;
  PackedArgs pk{nullptr, 0, 1};
  int Tp = 1;
  if (ps) if (int rc = packed_check_desc(who, desc, &unit)) return rc;
  if (int rc = tensor_check_desc(who, ps ? &unit : desc, n_entries, &bytes)) return rc;
  if (int rc = clip_check_desc(who, clip, desc, ps ? ps->patches : nullptr, ps != nullptr, &Tp)) return rc;
  if (!frames) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: no frame indices", who);
  const int T = clip->frames;
  for (int e = 0; e < n_entries; e++)
    for (int k = 0; k < T; k++)
      if (frames[(size_t)e * (size_t)T + (size_t)k] < 0)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: frame index %d (position %d of the clip)", who, e, frames[(size_t)e * (size_t)T + (size_t)k], k);
  if (int rc = check_orientations(who, "entry", orientations, n_entries)) return rc;
  if (ps) { if (int rc = clip_packed_check(who, desc, ps->samples, ps->patches, T, n_entries, out_bytes, &pk)) return rc; }
  else {
    if (bytes > (~(size_t)0) / (size_t)T) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: tensor too large", who);
    bytes *= (size_t)T;
    if (out_bytes < bytes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: out_bytes %zu is smaller than the tensor of %zu bytes", who, out_bytes, bytes);
  }
  // (everything above is decided without reading the handle)
  hipdec_batch* b = c->batch.get();
  for (int e = 0; e < n_entries; e++) {
    const int t = entries[e].item;
    if (t < 0 || t >= (int)c->frames.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d names track %d of %d", who, e, t, (int)c->frames.size());
    for (int k = 0; k < T; k++) {
      const int f = frames[(size_t)e * (size_t)T + (size_t)k];
      if (f >= (int)c->frames[(size_t)t].size())
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: frame index %d (position %d of the clip), track %d has %d frames", who, e, f, k, t, (int)c->frames[(size_t)t].size());
    }
  }
  DeviceScope scope(b->device);
  if (!ps && b->max_pixels && (uint64_t)desc->width * (uint64_t)desc->height > b->max_pixels)
    return set_error(HIPDEC_ERR_LIMIT, "%s: output of %d x %d pixels exceeds max_image_size_pixels", who, desc->width, desc->height);
  for (int e = 0; ps && b->max_pixels && e < n_entries; e++)
    if ((uint64_t)pk.samples[e].width * (uint64_t)pk.samples[e].height > b->max_pixels)
      return set_error(HIPDEC_ERR_LIMIT, "%s: entry %d: frames of %d x %d pixels exceed max_image_size_pixels", who, e, pk.samples[e].width, pk.samples[e].height);
  return guarded(who, [&]() -> int {
    hipStream_t s = follow_stream(b, stream);
    const size_t es = tensor_elem_bytes(desc->dtype);
    const bool nhwc = desc->layout == HIPDEC_TENSOR_NHWC, channel_major = clip->order == HIPDEC_CLIP_CHANNEL_MAJOR;
    color_tensor_begin();
    for (int e = 0; e < n_entries; e++) {
      hipdec_tensor_desc sample = *desc;
      uint64_t clip0 = 0;                                   // the clip's first element
      if (ps) { sample.width = pk.samples[e].width; sample.height = pk.samples[e].height; clip0 = pk.samples[e].offset; }
      const uint64_t W = (uint64_t)sample.width, H = (uint64_t)sample.height, frame_elems = 3ull * W * H;
      if (!ps) clip0 = (uint64_t)e * (uint64_t)T * frame_elems;
      const uint64_t P = (uint64_t)pk.patch, group_elems = (uint64_t)Tp * frame_elems;   // (the tokens of Tp frames: (h / P) * (w / P) of 3 * Tp * P * P elements)
      for (int k = 0; k < T; k++) {
        const hipdec_clips::Frame& fr = c->frames[(size_t)entries[e].item][(size_t)frames[(size_t)e * (size_t)T + (size_t)k]];
        const int i = fr.item;
        const PicParams& Pp = b->params[(size_t)i];
        const hipdec_image_info& I = b->pics[(size_t)i].info;
        int left, top, rw, rh;
        int rc = tensor_window(who, entries + e, e, Pp.out_width, Pp.out_height, &left, &top, &rw, &rh);
        hipdec_nclx nclx{1, I.colour_primaries, I.transfer_characteristics, I.matrix_coeffs, I.full_range_flag};
        // the frame's first element, the row pitch and the rows of a channel plane
        uint64_t at;
        int plane_rows = sample.height;
        if (pk.patch) at = clip0 + (uint64_t)(k / Tp) * group_elems + (uint64_t)(k % Tp) * P * P * (nhwc ? 3ull : 1ull);
        else if (channel_major) { at = clip0 + (uint64_t)k * W * H; plane_rows = T * sample.height; }
        else at = clip0 + (uint64_t)k * frame_elems;
        bool box = !clips_no_strided_box();   // (in: the call may take k_clip_box; the frames that do are counted where the launch goes out, color.hip)
        if (!rc) rc = tensor_record_entry(who, b->arena + Pp.off_out[0], Pp.out_stride[0], b->arena + Pp.off_out[1], Pp.out_stride[1], b->arena + Pp.off_out[2], Pp.out_stride[2],
                                          Pp.out_width, Pp.out_height, b->wide ? I.bit_depth_luma : 8, Pp.chroma_format_idc, &nclx, &nclx, &sample, left, top, rw, rh,
                                          entries[e].flip, (uint8_t*)out_dev + (size_t)at * es, orientations ? orientations[e] : 0, (size_t)W * (nhwc ? 3 : 1), plane_rows,
                                          pk.patch, pk.merge, Tp, &box);
        if (rc) {
          color_tensor_abort();
          const std::string why = hipdec_last_error();
          return why.find("entry ") != std::string::npos ? rc : set_error(rc, "%s: entry %d: %s", who, e, why.c_str());
        }
      }
    }
    const size_t slot = b->runs ? (b->runs - 1) % (b->ev.size() / kEv) : 0;
    hipEvent_t* ev = b->ev.data() + kEv * slot;
    HIPDEC_CHECK_HIP(hipEventRecord(ev[6], s));
    int rc = color_tensor_launch(ps ? b->color_packed : b->color_oriented, desc->filter, desc->dtype, s);
    HIPDEC_CHECK_HIP(hipEventRecord(ev[7], s));
    if (!rc && b->runs) b->colour_timed[slot] = 1;
    b->mark_done(s);
    if (!rc) g_clips_tensor_calls++;
    return rc;
  });
}

}  // namespace

extern "C" {

int hipdec_clips_create(hipdec_clips** out, int n_tracks, const int* sample_counts, const void* const* samples, const size_t* sample_sizes, uint64_t max_image_size_pixels)
{
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_create: NULL out");
  *out = nullptr;
  if (!sample_counts || !samples || !sample_sizes) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_create: NULL sample_counts, samples or sample_sizes");
  if (n_tracks <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_create: %d tracks", n_tracks);
  return guarded("clips_create", [&]() -> int {
    // what the arguments alone decide
    int64_t total = 0;
    std::vector<int> first((size_t)n_tracks), count((size_t)n_tracks);
    for (int t = 0; t < n_tracks; t++) {
      if (sample_counts[t] <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_create: track %d: %d samples", t, sample_counts[t]);
      first[(size_t)t] = (int)total; count[(size_t)t] = sample_counts[t];
      total += sample_counts[t];
      (void)chain_window_us();   // (reads HIPDEC_CHAIN_MAX_PICTURES once)
      if (total > g_chains.max_pictures)
        return set_error(HIPDEC_ERR_LIMIT, "clips_create: track %d: more than %ld samples in all (the chain limit, HIPDEC_CHAIN_MAX_PICTURES)", t, g_chains.max_pictures);
    }
    // the framing of every sample, as hipdec_decoder_push_data validates it
    for (int t = 0; t < n_tracks; t++)
      for (int i = 0; i < count[(size_t)t]; i++) {
        const uint8_t* p = (const uint8_t*)samples[first[(size_t)t] + i];
        const size_t size = sample_sizes[first[(size_t)t] + i];
        if (!p || !size) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_create: track %d, sample %d: no data", t, i);
        for (size_t ptr = 0; ptr < size;) {
          if (size - ptr < 4) return set_error(HIPDEC_ERR_END_OF_DATA, "clips_create: track %d, sample %d: truncated NAL length field", t, i);
          const uint32_t n = ((uint32_t)p[ptr] << 24) | ((uint32_t)p[ptr + 1] << 16) | ((uint32_t)p[ptr + 2] << 8) | p[ptr + 3];
          ptr += 4;
          if (n > size - ptr) return set_error(HIPDEC_ERR_END_OF_DATA, "clips_create: track %d, sample %d: NAL size exceeds the sample", t, i);
          ptr += n;
        }
      }
    // the samples as the front end takes them: one access unit each, the track's parameter sets in front (SampleQueue, as hipdec_decoder_push_data queues them)
    std::vector<std::vector<uint8_t>> blobs((size_t)total);
    for (int t = 0; t < n_tracks; t++) {
      SampleQueue sq;
      sq.first_closed = true;   // (no still in front: every sample is a sample of the sequence)
      for (int i = 0; i < count[(size_t)t]; i++) {
        sq.push((const uint8_t*)samples[first[(size_t)t] + i], sample_sizes[first[(size_t)t] + i]);
        sq.last_open = false;   // (the next sample is the next access unit whatever it starts with)
        if (sq.queue.size() != (size_t)i + 1 || !sq.queue.back().has_vcl)
          return set_error(HIPDEC_ERR_BITSTREAM, "clips_create: track %d, sample %d: not exactly one coded picture", t, i);
      }
      for (int i = 0; i < count[(size_t)t]; i++) blobs[(size_t)(first[(size_t)t] + i)] = std::move(sq.queue[(size_t)i].blob);
    }
    std::vector<const void*> ptrs((size_t)total);
    std::vector<size_t> sizes((size_t)total);
    for (size_t i = 0; i < (size_t)total; i++) { ptrs[i] = blobs[i].data(); sizes[i] = blobs[i].size(); }
    std::vector<SeqContext> fresh((size_t)n_tracks);
    std::vector<const SeqContext*> seqs((size_t)n_tracks);
    for (int t = 0; t < n_tracks; t++) seqs[(size_t)t] = &fresh[(size_t)t];
    int bad = -1;
    const ChainPlan plan{n_tracks, first.data(), count.data(), seqs.data(), &bad};
    std::unique_ptr<hipdec_clips> c(new hipdec_clips());
    c->batch.reset(new hipdec_batch());
    hipdec_batch& b = *c->batch;
    bool planned = false;
    // the plan has passed: only now is a device touched
    const std::function<int(const hipdec_batch&)> init = [&](const hipdec_batch&) -> int { planned = true; return ensure_init(); };
    if (int rc = build_batch(b, (int)total, ptrs.data(), sizes.data(), max_image_size_pixels, nullptr, nullptr, &plan, &init)) {
      if (planned) return rc;
      std::string why = hipdec_last_error();
      if (bad >= 0) {
        const size_t cut = why.find("sample ");   // (the plan's "track t of the launch set, sample i of the chain: ...")
        return set_error(rc, "clips_create: track %d, %s", bad, cut == std::string::npos ? why.c_str() : why.c_str() + cut);
      }
      // the combination was refused (8-bit beside wider tracks): the first track that differs from track 0
      int odd = 0;
      for (int t = 1; t < n_tracks && !odd; t++)
        if (!b.tracks[(size_t)t].items.empty() && !b.tracks[0].items.empty()) {
          const hipdec_image_info &A = b.pics[(size_t)b.tracks[0].items[0]].info, &B = b.pics[(size_t)b.tracks[(size_t)t].items[0]].info;
          if ((A.bit_depth_luma > 8 || A.bit_depth_chroma > 8) != (B.bit_depth_luma > 8 || B.bit_depth_chroma > 8)) odd = t;
        }
      return set_error(rc, "clips_create: track %d: %s", odd, why.c_str());
    }
    if (b.pics.empty()) return set_error(HIPDEC_ERR_BITSTREAM, "clips_create: track 0: no picture to decode");
    b.borrowed = true;
    c->device = b.device;
    // output order: coded video sequence by coded video sequence (an IDR picture behind the first picture starts one), each in POC order
    c->frames.resize((size_t)n_tracks);
    uint64_t n_frames = 0;
    for (int t = 0; t < n_tracks; t++) {
      const BatchLayout::ChainTrack& tr = b.tracks[(size_t)t];
      std::vector<hipdec_clips::Frame>& fs = c->frames[(size_t)t];
      int sequence = 0;
      for (size_t k = 0; k < tr.items.size(); k++) {
        const ParsedPicture& pp = b.pics[(size_t)tr.items[k]];
        if (pp.is_idr && k) sequence++;
        if (!pp.pic_output) continue;
        hipdec_clips::Frame f;
        f.item = tr.items[k]; f.sample = tr.samples[k]; f.poc = pp.poc; f.sequence = sequence;
        fs.push_back(f);
      }
      std::stable_sort(fs.begin(), fs.end(), [](const hipdec_clips::Frame& x, const hipdec_clips::Frame& y) { return x.sequence != y.sequence ? x.sequence < y.sequence : x.poc < y.poc; });
      n_frames += fs.size();
    }
    g_clips_sets++; g_clips_tracks += (uint64_t)n_tracks; g_clips_frames += n_frames;
    *out = c.release();
    return 0;
  });
}

void hipdec_clips_free(hipdec_clips* c) { delete c; }

int hipdec_clips_run(hipdec_clips* c, void* stream)
{
  if (!c) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_run: NULL object");
  hipdec_batch* b = c->batch.get();
  b->borrowed = false;   // (the owner's run)
  const int rc = hipdec_batch_run(b, stream);
  b->borrowed = true;
  return rc;
}

int hipdec_clips_status(hipdec_clips* c)
{
  if (!c) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_status: NULL object");
  return hipdec_batch_status(c->batch.get());
}

int hipdec_clips_track_count(const hipdec_clips* c)
{
  if (!c) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_track_count: NULL object");
  return (int)c->frames.size();
}
int hipdec_clips_frame_count(const hipdec_clips* c, int track)
{
  if (!c || track < 0 || track >= (int)c->frames.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_frame_count: bad arguments (track %d)", track);
  return (int)c->frames[(size_t)track].size();
}

int hipdec_clips_frame(const hipdec_clips* c, int track, int frame, hipdec_clip_frame* out)
{
  if (!c || !out || track < 0 || track >= (int)c->frames.size() || frame < 0 || frame >= (int)c->frames[(size_t)track].size())
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clips_frame: bad arguments (track %d, frame %d)", track, frame);
  const hipdec_clips::Frame& f = c->frames[(size_t)track][(size_t)frame];
  out->item = f.item; out->sample = f.sample; out->poc = f.poc; out->sequence = f.sequence;
  out->info = c->batch->pics[(size_t)f.item].info;
  return 0;
}

int hipdec_clips_frame_plane(hipdec_clips* c, int track, int frame, int plane, const void** dptr, size_t* stride)
{
  hipdec_clip_frame f;
  if (int rc = hipdec_clips_frame(c, track, frame, &f)) return rc;
  return hipdec_batch_device_plane(c->batch.get(), f.item, plane, dptr, stride);
}

int hipdec_clips_read_plane(hipdec_clips* c, int track, int frame, int plane, void* dst_host, size_t dst_stride)
{
  hipdec_clip_frame f;
  if (int rc = hipdec_clips_frame(c, track, frame, &f)) return rc;
  return hipdec_batch_read_plane(c->batch.get(), f.item, plane, dst_host, dst_stride);
}

hipdec_batch* hipdec_clips_batch(hipdec_clips* c) { return c ? c->batch.get() : nullptr; }

void hipdec_clips_stats(uint64_t* sets, uint64_t* tracks, uint64_t* frames, uint64_t* tensor_calls, uint64_t* strided_box_entries)
{
  if (sets) *sets = g_clips_sets.load();
  if (tracks) *tracks = g_clips_tracks.load();
  if (frames) *frames = g_clips_frames.load();
  if (tensor_calls) *tensor_calls = g_clips_tensor_calls.load();
  if (strided_box_entries) *strided_box_entries = clip_box_entries();
}

int hipdec_clips_to_tensor(hipdec_clips* c, const hipdec_tensor_desc* desc, const hipdec_clip_desc* clip, const hipdec_tensor_entry* entries, const int* frames,
                           const int* orientations, int n_entries, void* out_dev, size_t out_bytes, void* stream)
{
  return clips_to_tensor_impl(c, desc, clip, entries, frames, orientations, n_entries, out_dev, out_bytes, stream, nullptr);
}

int hipdec_clips_to_tensor_packed(hipdec_clips* c, const hipdec_tensor_desc* desc, const hipdec_clip_desc* clip, const hipdec_tensor_entry* entries, const int* frames,
                                  const int* orientations, const hipdec_tensor_sample* samples, const hipdec_tensor_patches* patches, int n_entries, void* out_dev,
                                  size_t out_bytes, void* stream)
{
  const PackedSpec ps{samples, patches};
  return clips_to_tensor_impl(c, desc, clip, entries, frames, orientations, n_entries, out_dev, out_bytes, stream, &ps);
}

int hipdec_clip_packed_layout(const hipdec_clip_desc* clip, const hipdec_tensor_patches* patches, const int* widths, const int* heights, int n, uint64_t* offsets,
                              uint32_t* tokens, uint64_t* total_elements)
{
  const char* who = "clip_packed_layout";
  if (!widths || !heights || n < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who), -1;
  if (packed_check_patches(who, patches)) return -1;
  int Tp = 1;
  if (clip_check_desc(who, clip, nullptr, patches, true, &Tp)) return -1;
  const int patch = patches ? patches->patch : 0, merge = patches ? patches->merge : 1;
  uint64_t at = 0;
  for (int e = 0; e < n; e++) {
    if (packed_check_size(who, e, widths[e], heights[e], patch, merge)) return -1;
    const uint64_t wh = (uint64_t)widths[e] * (uint64_t)heights[e];
    const uint64_t tok = patch ? (uint64_t)(clip->frames / Tp) * (uint64_t)(widths[e] / patch) * (uint64_t)(heights[e] / patch) : 0;
    if (wh > (~0ull) / (3ull * (uint64_t)clip->frames) || tok > 0xffffffffull || 3ull * (uint64_t)clip->frames * wh > ~0ull - at)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: the sequence is too long", who, e), -1;
    if (offsets) offsets[e] = at;
    if (tokens) tokens[e] = (uint32_t)tok;
    at += 3ull * (uint64_t)clip->frames * wh;
  }
  if (total_elements) *total_elements = at;
  return 0;
}

}  // extern "C"
