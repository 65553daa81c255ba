/* decode_batch.c — a throughput host over the C ABI (include/heif_hipdec.h): a stream of batches of independent HEVC-intra items, each
 * item in libheif's plugin framing ([4-byte big-endian length][NAL unit]..., parameter sets first — what push_data2 receives,
 * libheif/plugins/decoder_libde265.cc:322-368).  Every batch takes over its predecessor's arena, so the host work of batch k + 1 (header parsing,
 * staging, upload) overlaps the kernels of batch k; the decoded planes and the interleaved RGB stay in HBM until they are read.
 *
 *   cc -I include examples/decode_batch.c -L libheif_amd -lheifhip -Wl,-rpath,$PWD/libheif_amd -o decode_batch
 *   ./decode_batch item0.hevc item1.hevc ...          (files as written by tools/streamgen.py, or dumped from a HEIC's hvcC + item data)
 *   ./decode_batch --thumb 256 item0.hevc ...         ends in ONE launch that turns every item into an RGB24 preview that fits into 256 x 256
 *                                                     (the size rule of libheif's examples/heif_thumbnailer.cc:172-186, area-averaged on the device)
 *   ./decode_batch --thumb 256 --orient 1 item0.hevc  the previews as they are DISPLAYED for orientation code 0 .. 7 (hipdec_orientation: what the host folded the
 *                                                     items' 'irot' / 'imir' into with hipdec_orientation_compose), still ONE launch: the rotation is in its store
 *   ./decode_batch --thumb 448 --patches 14:2 ...      instead of previews, ONE launch writes the batch as the packed sequence of patch tokens native-resolution
 *                                                     vision encoders take (hipdec_batch_to_tensor_packed): every item at its own preview size rounded down to a
 *                                                     multiple of P * M, uint8 tokens of 3 * P * P elements in Conv2d weight order, merge groups of M x M;
 *                                                     last among the --thumb options
 *   ./decode_batch --thumb 256 --filter bicubic ...   the previews with another filter: box (the default) | nearest | bilinear | bicubic - the last two are
 *                                                     PIL.Image.resize bit for bit (HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC); after --orient where both are given
 *   ./decode_batch --thumb 256 --warp 15 item0.hevc   the previews rotated by 15 degrees counter-clockwise about their centre, exactly as PIL.Image.rotate(15,
 *                                                     BILINEAR) turns the resized 8-bit preview (hipdec_batch_to_tensor_warped with hipdec_rotate_map): per
 *                                                     preview one resize launch and one warp launch, black outside; after --orient / --filter, not with --patches
 *   ./decode_batch --thumb 256 --photo contrast 1.3 item0.hevc   the previews through one photometric operation, exactly as PIL.ImageEnhance / ImageOps
 *                                                     change the resized 8-bit preview (hipdec_batch_to_tensor_photo): OP is brightness | color | contrast |
 *                                                     sharpness | posterize | solarize | invert | autocontrast | equalize, VALUE its factor, bits or
 *                                                     threshold (0 for the last three); after --orient / --filter, not with --warp or --patches
 *   ./decode_batch --tensor 224 item0.hevc ...        ends in ONE launch that writes a float16 N x 3 x 224 x 224 tensor: the centred square of every item,
 *                                                     area-averaged, (V / 255 - mean) / std with the usual ImageNet constants
 *   ./decode_batch --thumb 256 --hue 43 --blur 1.5 item0.hevc    the previews through Pillow's hue shift (D of 0 .. 255 added to H of convert("HSV")) and / or
 *                                                     PIL.ImageFilter.GaussianBlur(RADIUS), RADIUS 0 .. 8, bit for bit (hipdec_batch_to_tensor_augmented)
 *   ./decode_batch --thumb 256 --recipe 15 color 1.4 item0.hevc   the previews rotated by ANGLE degrees (BILINEAR, black outside) and then through one photometric
 *                                                     operation, both steps in ONE chain, as RandAugment draws them (hipdec_batch_to_tensor_recipe): OP and
 *                                                     VALUE as for --photo; a statistics operation (contrast, autocontrast, equalize) sees the fill pixels
 *   ./decode_batch --thumb 256 --frame 256 224 item0.hevc   instead of previews, ONE launch writes the evaluation batch: every item resized so that its shorter
 *                                                     side is RESIZE, then the centred CROP x CROP square of it - torchvision's Resize(RESIZE) -> CenterCrop(CROP),
 *                                                     hipdec_resize_crop_place and hipdec_batch_to_tensor_framed - as a uint8 N x CROP x CROP x 3 tensor; only the
 *                                                     square is computed, an item smaller than it is padded with black; RESIZE takes the place of --thumb's N;
 *                                                     after --orient / --filter, not with the options above
 *   ./decode_batch --thumb 96 --sheet 4 3 item0.hevc ...   instead of previews, ONE launch set writes a contact sheet: COLS x ROWS cells of N x N with 2 pixels
 *                                                     between them, item k letterboxed into cell k (hipdec_sheet_tiles, hipdec_batch_to_tensor_composed),
 *                                                     white elsewhere, as ONE uint8 H x W x 3 picture; at most COLS * ROWS items; where --frame may stand
 *   ./decode_batch --album 16 6x8 tile0.hevc ...      the items are TILES: 16 grid photos of 6 x 8 tiles (tile t of photo k is item (k * 48 + t) mod n; the
 *                                                     output is the whole tiled area) composed by ONE launch set and ONE paste launch; prints Mpixel/s
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "heif_hipdec.h"

static void* slurp(const char* path, size_t* size)
{
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc(n > 0 ? (size_t)n : 1);
  if (p && fread(p, 1, (size_t)n, f) != (size_t)n) { free(p); p = NULL; }
  fclose(f);
  *size = (size_t)n;
  return p;
}

/* K grid photos of rows x cols tiles as one album: create, then run + status three times (the first loads code objects), the last one timed */
static int run_album(int k_photos, int rows, int cols, int n, const void** data, const size_t* sizes)
{
  hipdec_image_info tile;
  if (hipdec_probe(data[0], sizes[0], 0, &tile)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
  const int per = rows * cols, n_tiles = k_photos * per;
  hipdec_album_photo* photos = (hipdec_album_photo*)calloc((size_t)k_photos, sizeof(hipdec_album_photo));
  const void** tiles = (const void**)calloc((size_t)n_tiles, sizeof(void*));
  size_t* tile_sizes = (size_t*)calloc((size_t)n_tiles, sizeof(size_t));
  for (int t = 0; t < n_tiles; t++) { tiles[t] = data[t % n]; tile_sizes[t] = sizes[t % n]; }
  for (int k = 0; k < k_photos; k++) {
    photos[k].rows = rows; photos[k].cols = cols; photos[k].first_tile = k * per;
    photos[k].out_width = cols * tile.width; photos[k].out_height = rows * tile.height;
  }
  hipdec_album* a = NULL;
  if (hipdec_album_create(&a, k_photos, photos, tiles, tile_sizes, n_tiles, 0)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
  double ms = 0;
  for (int step = 0; step < 3; step++) {
    struct timespec t0, t1;
    timespec_get(&t0, TIME_UTC);
    if (hipdec_album_run(a, NULL) || hipdec_album_status(a)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
    timespec_get(&t1, TIME_UTC);
    ms = (double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) / 1e6;
  }
  const double mpix = (double)k_photos * photos[0].out_width * photos[0].out_height / 1e6;
  const size_t es = tile.bit_depth_luma > 8 ? 2 : 1, row = (size_t)photos[0].out_width * es;
  uint8_t* y = (uint8_t*)malloc(row * (size_t)photos[0].out_height);
  if (!y || hipdec_album_read_plane(a, k_photos - 1, 0, y, row)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
  unsigned long long sum = 0;
  for (size_t i = 0; i < row * (size_t)photos[0].out_height; i++) sum += y[i];
  uint64_t albums = 0, n_photos = 0, pastes = 0;
  hipdec_album_stats(&albums, &n_photos, &pastes);
  printf("album: %d photos of %d x %d tiles, %dx%d each: %.2f ms, %.0f Mpixel/s of composed photos; %llu paste launches for %llu runs; luma byte sum of the last photo %llu\n",
         k_photos, rows, cols, photos[0].out_width, photos[0].out_height, ms, mpix / ms * 1e3, (unsigned long long)pastes, 3ull, sum);
  free(y); free(photos); free(tiles); free(tile_sizes);
  hipdec_album_free(a);
  hipdec_shutdown();
  return 0;
}

int main(int argc, char** argv)
{
  const char* prog = argv[0];
  int album = 0, album_rows = 0, album_cols = 0;
  if (argc >= 2 && !strcmp(argv[1], "--album")) {
    album = argc >= 4 ? atoi(argv[2]) : 0;
    if (album < 1 || sscanf(argv[3], "%dx%d", &album_rows, &album_cols) != 2 || album_rows < 1 || album_cols < 1 || album_rows > 256 || album_cols > 256) argc = 0;
    else { argv += 3; argc -= 3; }
  }
  int thumb = 0;
  if (argc >= 2 && !strcmp(argv[1], "--thumb")) {
    thumb = argc >= 3 ? atoi(argv[2]) : 0;
    if (thumb < 1) argc = 0;                                       /* no or a bad N: usage */
    else { argv += 2; argc -= 2; }
  }
  int orient = -1;                                                 /* -1: the unoriented call */
  if (thumb && argc >= 2 && !strcmp(argv[1], "--orient")) {
    orient = argc >= 3 ? atoi(argv[2]) : -1;
    if (orient < 0 || orient > 7 || (argv[2][0] < '0' || argv[2][0] > '7') || argv[2][1]) argc = 0;
    else { argv += 2; argc -= 2; }
  }
  int filter = HIPDEC_SCALE_BOX;
  if (thumb && argc >= 2 && !strcmp(argv[1], "--filter")) {
    static const struct { const char* name; int value; } filters[4] = {{"box", HIPDEC_SCALE_BOX}, {"nearest", HIPDEC_SCALE_NEAREST}, {"bilinear", HIPDEC_SCALE_BILINEAR},
                                                                      {"bicubic", HIPDEC_SCALE_BICUBIC}};
    int k = 4;
    if (argc >= 3) for (k = 0; k < 4 && strcmp(argv[2], filters[k].name); k++) {}
    if (k == 4) argc = 0;                                          /* no or an unknown name: usage */
    else { filter = filters[k].value; argv += 2; argc -= 2; }
  }
  int warp = 0;
  double warp_angle = 0.0;
  if (thumb && argc >= 2 && !strcmp(argv[1], "--warp")) {
    char* end = NULL;
    warp_angle = argc >= 3 ? strtod(argv[2], &end) : 0.0;
    if (argc < 3 || end == argv[2] || *end || warp_angle < -36000.0 || warp_angle > 36000.0) argc = 0;   /* no or a bad ANGLE: usage */
    else { warp = 1; argv += 2; argc -= 2; }
  }
  int photo = 0;
  double photo_value = 0.0;
  if (thumb && !warp && argc >= 2 && !strcmp(argv[1], "--photo")) {
    static const char* const ops[] = {"brightness", "color", "contrast", "sharpness", "posterize", "solarize", "invert", "autocontrast", "equalize"};
    char* end = NULL;
    for (int k = 0; argc >= 3 && k < 9; k++) if (!strcmp(argv[2], ops[k])) photo = HIPDEC_PHOTO_BRIGHTNESS + k;
    photo_value = argc >= 4 ? strtod(argv[3], &end) : 0.0;
    if (!photo || argc < 4 || end == argv[3] || *end) argc = 0;    /* no or an unknown OP, no or a bad VALUE: usage (the library checks the value's range) */
    else { argv += 3; argc -= 3; }
  }
  int recipe = 0;                                                 /* --recipe ANGLE OP VALUE: rotate, then one photometric operation, one chain */
  double recipe_angle = 0.0, recipe_value = 0.0;
  if (thumb && !warp && !photo && argc >= 2 && !strcmp(argv[1], "--recipe")) {
    static const char* const ops[] = {"brightness", "color", "contrast", "sharpness", "posterize", "solarize", "invert", "autocontrast", "equalize"};
    char *end_a = NULL, *end_v = NULL;
    recipe_angle = argc >= 3 ? strtod(argv[2], &end_a) : 0.0;
    for (int k = 0; argc >= 4 && k < 9; k++) if (!strcmp(argv[3], ops[k])) recipe = HIPDEC_PHOTO_BRIGHTNESS + k;
    recipe_value = argc >= 5 ? strtod(argv[4], &end_v) : 0.0;
    if (!recipe || argc < 5 || end_a == argv[2] || *end_a || recipe_angle < -36000.0 || recipe_angle > 36000.0 || end_v == argv[4] || *end_v) argc = 0;
    else { argv += 4; argc -= 4; }
  }
  int augment = 0;                                                /* --hue D and / or --blur RADIUS: a chain of the augment stage, in that order */
  double hue = -1.0, blur = -1.0;
  while (thumb && !warp && !photo && !recipe && argc >= 2 && (!strcmp(argv[1], "--hue") || !strcmp(argv[1], "--blur"))) {
    char* end = NULL;
    const double v = argc >= 3 ? strtod(argv[2], &end) : 0.0;
    if (argc < 3 || end == argv[2] || *end) { argc = 0; break; }  /* no or a bad value: usage (the library checks the range) */
    if (!strcmp(argv[1], "--hue")) hue = v; else blur = v;
    augment = 1; argv += 2; argc -= 2;
  }
  int patch = 0, merge = 1;
  if (thumb && !warp && !photo && !recipe && !augment && argc >= 2 && !strcmp(argv[1], "--patches")) {
    char tail = 0;
    const int got = argc >= 3 ? sscanf(argv[2], "%d:%d%c", &patch, &merge, &tail) : 0;
    if ((got != 1 && got != 2) || patch < 1 || patch > 256 || merge < 1 || merge > 16) argc = 0;   /* no or a bad P[:M]: usage */
    else { argv += 2; argc -= 2; }
  }
  int frame_resize = 0, frame_crop = 0;
  if (thumb && !warp && !photo && !recipe && !augment && !patch && argc >= 2 && !strcmp(argv[1], "--frame")) {
    frame_resize = argc >= 3 ? atoi(argv[2]) : 0;
    frame_crop = argc >= 4 ? atoi(argv[3]) : 0;
    if (frame_resize < 1 || frame_crop < 1) argc = 0;             /* no or a bad RESIZE / CROP: usage */
    else { argv += 3; argc -= 3; }
  }
  int sheet_cols = 0, sheet_rows = 0;
  if (thumb && !warp && !photo && !recipe && !augment && !patch && !frame_resize && argc >= 2 && !strcmp(argv[1], "--sheet")) {
    sheet_cols = argc >= 3 ? atoi(argv[2]) : 0;
    sheet_rows = argc >= 4 ? atoi(argv[3]) : 0;
    if (sheet_cols < 1 || sheet_rows < 1 || sheet_cols > 1024 || sheet_rows > 1024 || argc - 4 > sheet_cols * sheet_rows) argc = 0;   /* no or bad COLS / ROWS, too many items: usage */
    else { argv += 3; argc -= 3; }
  }
  int tensor = 0;
  if (!thumb && argc >= 2 && !strcmp(argv[1], "--tensor")) {
    tensor = argc >= 3 ? atoi(argv[2]) : 0;
    if (tensor < 1) argc = 0;
    else { argv += 2; argc -= 2; }
  }
  if (argc < 2) { fprintf(stderr, "usage: %s [--thumb N [--orient CODE] [--filter box|nearest|bilinear|bicubic] [--warp ANGLE | --photo OP VALUE | --recipe ANGLE OP VALUE | [--hue D] [--blur RADIUS] | --patches P[:M] | --frame RESIZE CROP | --sheet COLS ROWS] | --tensor N | --album K ROWSxCOLS] item.hevc [item.hevc ...]\n", prog); return 2; }
  const int n = argc - 1;
  const void** data = (const void**)calloc((size_t)n, sizeof(void*));
  size_t* sizes = (size_t*)calloc((size_t)n, sizeof(size_t));
  for (int i = 0; i < n; i++) {
    data[i] = slurp(argv[1 + i], &sizes[i]);
    if (!data[i]) { fprintf(stderr, "cannot read %s\n", argv[1 + i]); return 2; }
    hipdec_image_info info;
    int rc = hipdec_probe(data[i], sizes[i], 0, &info);            /* host-only: headers, limits, unsupported tools */
    if (rc) { fprintf(stderr, "%s: %s\n", argv[1 + i], hipdec_last_error()); return 1; }
  }
  hipdec_set_arena_cache_bytes((size_t)64 << 30);                  /* keep two large arenas parked instead of hipFree()ing them */
  if (album) return run_album(album, album_rows, album_cols, n, data, sizes);
  hipdec_batch* prev = NULL;
  for (int step = 0; step < 3; step++) {                           /* the same items three times: a stand-in for a stream of batches */
    hipdec_batch* b = NULL;
    int rc = hipdec_batch_create_recycling(&b, n, data, sizes, 0, prev);   /* parses + stages + uploads; overlaps prev's kernels */
    if (!rc) rc = hipdec_batch_run(b, NULL);                       /* asynchronous: CABAC, residual, reconstruction, deblock, SAO */
    if (rc) { fprintf(stderr, "batch %d: %s\n", step, hipdec_last_error()); return 1; }
    if (prev) {
      if (hipdec_batch_status(prev)) { fprintf(stderr, "batch %d failed on the device: %s\n", step - 1, hipdec_last_error()); return 1; }
      hipdec_batch_free(prev);
    }
    prev = b;
  }
  if (hipdec_batch_status(prev)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
  for (int i = 0; i < n; i++) {
    hipdec_image_info info;
    hipdec_batch_info(prev, i, &info);
    const size_t es = info.bit_depth_luma > 8 ? 2 : 1;
    uint8_t* y = (uint8_t*)malloc((size_t)info.width * info.height * es);
    if (hipdec_batch_read_plane(prev, i, 0, y, (size_t)info.width * es)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
    unsigned long long sum = 0;
    for (size_t k = 0; k < (size_t)info.width * info.height * es; k++) sum += y[k];
    printf("%s: %dx%d, %d bit, luma byte sum %llu\n", argv[1 + i], info.width, info.height, info.bit_depth_luma, sum);
    free(y);
  }
  if (thumb) {                                                     /* previews of all items as one launch: no full-size RGB exists anywhere, and of the colour stage only the previews cross to the host */
    int* ws = (int*)calloc((size_t)n, sizeof(int));
    int* hs = (int*)calloc((size_t)n, sizeof(int));
    int* codes = (int*)calloc((size_t)n, sizeof(int));
    if (frame_resize) {                                            /* Resize -> CenterCrop of the whole batch: one framed call, one tensor */
      hipdec_tensor_desc d;
      memset(&d, 0, sizeof d);
      d.width = d.height = frame_crop; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
      for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
      hipdec_tensor_place* pl = (hipdec_tensor_place*)calloc((size_t)n, sizeof(hipdec_tensor_place));
      for (int i = 0; i < n; i++) {
        hipdec_image_info info;
        hipdec_batch_info(prev, i, &info);
        const int turned = orient > 0 && (orient & 1);             /* the rule sees the DISPLAYED picture */
        codes[i] = orient > 0 ? orient : 0;
        if (hipdec_resize_crop_place(turned ? info.height : info.width, turned ? info.width : info.height, frame_resize, frame_crop, frame_crop, pl + i)) {
          fprintf(stderr, "%s\n", hipdec_last_error());
          return 1;
        }
      }
      const size_t bytes = hipdec_tensor_bytes(&d, n), each = bytes / (size_t)n;
      void* t = bytes ? hipdec_malloc(bytes) : NULL;
      uint8_t* host = (uint8_t*)malloc(bytes ? bytes : 1);
      if (!t || !host || hipdec_batch_to_tensor_framed(prev, &d, NULL, codes, pl, NULL, NULL, n, t, bytes, NULL) || hipdec_batch_status(prev) ||
          hipdec_memcpy_d2h(host, t, bytes)) {
        fprintf(stderr, "%s\n", hipdec_last_error());
        return 1;
      }
      for (int i = 0; i < n; i++) {
        unsigned long long sum = 0;
        for (size_t k = 0; k < each; k++) sum += host[(size_t)i * each + k];
        printf("%s: %dx%d of the sample resized to %dx%d, at (%d, %d), byte sum %llu\n", argv[1 + i], frame_crop, frame_crop, pl[i].width, pl[i].height, -pl[i].x, -pl[i].y, sum);
      }
      uint64_t tiles = 0, skipped = 0;
      hipdec_framed_stats(NULL, NULL, &tiles, &skipped);
      printf("framed tensor %dx%dx%dx3 uint8: %llu tiles computed, %llu skipped\n", n, frame_crop, frame_crop, (unsigned long long)tiles, (unsigned long long)skipped);
      free(host); hipdec_free(t); free(pl);
      free(ws); free(hs); free(codes);
      hipdec_batch_free(prev);
      hipdec_shutdown();
      return 0;
    }
    if (sheet_cols) {                                              /* a contact sheet of the whole batch: one composed call, one picture */
      const int gap = 2;
      hipdec_tensor_desc d;
      memset(&d, 0, sizeof d);
      d.width = sheet_cols * thumb + (sheet_cols - 1) * gap; d.height = sheet_rows * thumb + (sheet_rows - 1) * gap;
      d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
      for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
      hipdec_tensor_tile* tiles = (hipdec_tensor_tile*)calloc((size_t)n, sizeof(hipdec_tensor_tile));
      for (int i = 0; i < n; i++) {
        hipdec_image_info info;
        hipdec_batch_info(prev, i, &info);
        const int turned = orient > 0 && (orient & 1);             /* a cell holds the DISPLAYED picture */
        codes[i] = orient > 0 ? orient : 0;
        ws[i] = turned ? info.height : info.width; hs[i] = turned ? info.width : info.height;
      }
      hipdec_tensor_fill white;
      memset(&white, 0, sizeof white);
      white.value[0] = white.value[1] = white.value[2] = 255.0f; white.domain = HIPDEC_FILL_COMPONENT;
      const size_t bytes = hipdec_tensor_bytes(&d, 1);
      void* t = bytes ? hipdec_malloc(bytes) : NULL;
      uint8_t* host = (uint8_t*)malloc(bytes ? bytes : 1);
      if (!t || !host || hipdec_sheet_tiles(sheet_cols, sheet_rows, thumb, thumb, gap, ws, hs, n, 1, 0, tiles) ||
          hipdec_batch_to_tensor_composed(prev, &d, NULL, codes, tiles, &white, NULL, n, 1, t, bytes, NULL) || hipdec_batch_status(prev) ||
          hipdec_memcpy_d2h(host, t, bytes)) {
        fprintf(stderr, "%s\n", hipdec_last_error());
        return 1;
      }
      for (int i = 0; i < n; i++)
        printf("%s: cell %d, %dx%d at (%d, %d)\n", argv[1 + i], i, tiles[i].place.width, tiles[i].place.height, tiles[i].place.x, tiles[i].place.y);
      unsigned long long sum = 0;
      for (size_t k = 0; k < bytes; k++) sum += host[k];
      uint64_t pieces = 0, launches = 0;
      hipdec_composed_stats(NULL, NULL, &pieces, NULL, &launches);
      printf("contact sheet %dx%dx3 uint8, %d x %d cells: %llu pieces, %llu cover launch(es), byte sum %llu\n", d.height, d.width, sheet_cols, sheet_rows,
             (unsigned long long)pieces, (unsigned long long)launches, sum);
      free(host); hipdec_free(t); free(tiles);
      free(ws); free(hs); free(codes);
      hipdec_batch_free(prev);
      hipdec_shutdown();
      return 0;
    }
    void** outs = (void**)calloc((size_t)n, sizeof(void*));
    size_t* strides = (size_t*)calloc((size_t)n, sizeof(size_t));
    for (int i = 0; i < n; i++) {
      hipdec_image_info info;
      hipdec_batch_info(prev, i, &info);
      const int dw = orient > 0 && (orient & 1) ? info.height : info.width;   /* the size rule sees the DISPLAYED picture: a quarter turn swaps the sides */
      const int dh = orient > 0 && (orient & 1) ? info.width : info.height;
      ws[i] = dw; hs[i] = dh;
      codes[i] = orient > 0 ? orient : 0;
      if (dw > thumb || dh > thumb) {                              /* heif_thumbnailer.cc:172-186 */
        if (dw > dh) { hs[i] = (int)((long long)dh * thumb / dw); ws[i] = thumb; }
        else { ws[i] = (int)((long long)dw * thumb / dh); hs[i] = thumb; }
      }
      if (patch) { ws[i] -= ws[i] % (patch * merge); hs[i] -= hs[i] % (patch * merge); }   /* choosing the sizes is the caller's: here, rounded down */
      if (ws[i] < 1 || hs[i] < 1) { fprintf(stderr, "%s: zero thumbnail output size\n", argv[1 + i]); return 1; }
      if (patch) continue;
      strides[i] = (size_t)ws[i] * 3;
      outs[i] = hipdec_malloc(strides[i] * (size_t)hs[i]);
      if (!outs[i]) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
    }
    if (patch) {                                                   /* the packed sequence of the whole batch: one launch, one buffer */
      hipdec_tensor_desc d;
      memset(&d, 0, sizeof d);                                     /* width = height = 0: the sizes are per sample */
      d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NCHW; d.filter = filter;
      const hipdec_tensor_patches pt = {patch, merge, {0, 0}};
      uint64_t* offs = (uint64_t*)calloc((size_t)n, sizeof(uint64_t));
      uint32_t* toks = (uint32_t*)calloc((size_t)n, sizeof(uint32_t));
      hipdec_tensor_sample* sm = (hipdec_tensor_sample*)calloc((size_t)n, sizeof(hipdec_tensor_sample));
      uint64_t total = 0;
      if (hipdec_tensor_packed_layout(&pt, ws, hs, n, offs, toks, &total)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
      for (int i = 0; i < n; i++) { sm[i].width = ws[i]; sm[i].height = hs[i]; sm[i].offset = offs[i]; }
      void* seq = hipdec_malloc((size_t)total);
      uint8_t* host = (uint8_t*)malloc((size_t)total);
      if (!seq || !host || hipdec_batch_to_tensor_packed(prev, &d, NULL, codes, sm, &pt, n, seq, (size_t)total, NULL) || hipdec_batch_status(prev) ||
          hipdec_memcpy_d2h(host, seq, (size_t)total)) {
        fprintf(stderr, "%s\n", hipdec_last_error());
        return 1;
      }
      unsigned long long all = 0, tokens = 0;
      for (int i = 0; i < n; i++) {
        unsigned long long sum = 0;
        for (uint64_t k = 0; k < 3ull * (uint64_t)ws[i] * (uint64_t)hs[i]; k++) sum += host[offs[i] + k];
        printf("%s: %u tokens of %dx%d at %dx%d, byte sum %llu\n", argv[1 + i], toks[i], patch, patch, ws[i], hs[i], sum);
        all += sum; tokens += toks[i];
      }
      printf("packed sequence: %llu tokens x %d elements, byte sum %llu\n", tokens, 3 * patch * patch, all);
      free(host); hipdec_free(seq); free(offs); free(toks); free(sm);
      free(ws); free(hs); free(codes); free(outs); free(strides);
      hipdec_batch_free(prev);
      hipdec_shutdown();
      return 0;
    }
    int rc = 0;
    if (warp) {                                                    /* every preview has its own size: one warped call per preview, U8 / NHWC = RGB24 rows */
      for (int i = 0; i < n && !rc; i++) {
        hipdec_tensor_desc d;
        memset(&d, 0, sizeof d);
        d.width = ws[i]; d.height = hs[i]; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
        for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
        const hipdec_tensor_entry e = {i, 0, 0, 0, 0, 0};
        const hipdec_warp_desc wd = {ws[i], hs[i], HIPDEC_SCALE_BILINEAR, 0};
        hipdec_tensor_map map;
        rc = hipdec_rotate_map(warp_angle, ws[i], hs[i], &map);
        if (!rc) rc = hipdec_batch_to_tensor_warped(prev, &d, &e, codes + i, &wd, &map, NULL, 1, outs[i], strides[i] * (size_t)hs[i], NULL);
      }
    } else if (photo) {                                            /* likewise one photo call per preview: a resize launch, then the stage's launches */
      for (int i = 0; i < n && !rc; i++) {
        hipdec_tensor_desc d;
        memset(&d, 0, sizeof d);
        d.width = ws[i]; d.height = hs[i]; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
        for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
        const hipdec_tensor_entry e = {i, 0, 0, 0, 0, 0};
        const hipdec_photo_desc pd = {ws[i], hs[i], {0, 0}};
        hipdec_photo_chain chain;
        memset(&chain, 0, sizeof chain);
        chain.n_ops = 1; chain.ops[0].op = photo; chain.ops[0].value = photo_value;
        rc = hipdec_batch_to_tensor_photo(prev, &d, &e, codes + i, &pd, &chain, 1, outs[i], strides[i] * (size_t)hs[i], NULL);
      }
    } else if (recipe) {                                           /* one recipe call per preview: the rotation and the operation are steps of ONE chain */
      for (int i = 0; i < n && !rc; i++) {
        hipdec_tensor_desc d;
        memset(&d, 0, sizeof d);
        d.width = ws[i]; d.height = hs[i]; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
        for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
        const hipdec_tensor_entry e = {i, 0, 0, 0, 0, 0};
        const hipdec_photo_desc pd = {ws[i], hs[i], {0, 0}};
        hipdec_recipe_affine affine;
        memset(&affine, 0, sizeof affine);                         /* fill 0, 0, 0 */
        affine.filter = HIPDEC_SCALE_BILINEAR;
        rc = hipdec_rotate_map(recipe_angle, ws[i], hs[i], &affine.map);
        hipdec_augment_chain chain;
        memset(&chain, 0, sizeof chain);
        chain.n_ops = 2;
        chain.ops[0].op = HIPDEC_RECIPE_AFFINE; chain.ops[0].value = 0.0;   /* the index of `affine` among the call's records */
        chain.ops[1].op = recipe; chain.ops[1].value = recipe_value;
        if (!rc) rc = hipdec_batch_to_tensor_recipe(prev, &d, &e, codes + i, &pd, &chain, &affine, 1, 1, outs[i], strides[i] * (size_t)hs[i], NULL);
      }
    } else if (augment) {                                          /* and one augmented call per preview: hue, then Gaussian blur, as Pillow does them */
      for (int i = 0; i < n && !rc; i++) {
        hipdec_tensor_desc d;
        memset(&d, 0, sizeof d);
        d.width = ws[i]; d.height = hs[i]; d.dtype = HIPDEC_TENSOR_U8; d.layout = HIPDEC_TENSOR_NHWC; d.filter = filter;
        for (int c = 0; c < 3; c++) d.scale[c] = 1.0f;
        const hipdec_tensor_entry e = {i, 0, 0, 0, 0, 0};
        const hipdec_photo_desc pd = {ws[i], hs[i], {0, 0}};
        hipdec_augment_chain chain;
        memset(&chain, 0, sizeof chain);
        if (hue >= 0.0) { chain.ops[chain.n_ops].op = HIPDEC_AUGMENT_HUE; chain.ops[chain.n_ops++].value = hue; }
        if (blur >= 0.0) { chain.ops[chain.n_ops].op = HIPDEC_AUGMENT_GAUSSIAN_BLUR; chain.ops[chain.n_ops++].value = blur; }
        rc = hipdec_batch_to_tensor_augmented(prev, &d, &e, codes + i, &pd, &chain, 1, outs[i], strides[i] * (size_t)hs[i], NULL);
      }
    } else {
      rc = orient < 0 ? hipdec_batch_to_rgb_scaled_all(prev, 10, ws, hs, filter, (void* const*)outs, strides, NULL)
                      : hipdec_batch_to_rgb_scaled_oriented_all(prev, 10, codes, ws, hs, filter, (void* const*)outs, strides, NULL);
    }
    if (rc || hipdec_batch_status(prev)) {
      fprintf(stderr, "%s\n", hipdec_last_error());
      return 1;
    }
    for (int i = 0; i < n; i++) {
      const size_t bytes = strides[i] * (size_t)hs[i];
      uint8_t* rgb = (uint8_t*)malloc(bytes);
      if (!rgb || hipdec_memcpy_d2h(rgb, outs[i], bytes)) { fprintf(stderr, "%s\n", hipdec_last_error()); return 1; }
      unsigned long long sum = 0;
      for (size_t k = 0; k < bytes; k++) sum += rgb[k];
      printf("%s: preview %dx%d RGB24, byte sum %llu\n", argv[1 + i], ws[i], hs[i], sum);
      free(rgb);
      hipdec_free(outs[i]);
    }
    free(ws); free(hs); free(codes); free(outs); free(strides);
  }
  if (tensor) {                                                    /* the loader's batch tensor as one launch: crop, scale, normalise, float16 NCHW */
    static const float mean[3] = {0.485f, 0.456f, 0.406f}, std[3] = {0.229f, 0.224f, 0.225f};
    hipdec_tensor_desc d;
    memset(&d, 0, sizeof d);
    d.width = d.height = tensor; d.dtype = HIPDEC_TENSOR_F16; d.layout = HIPDEC_TENSOR_NCHW; d.filter = HIPDEC_SCALE_BOX;
    for (int c = 0; c < 3; c++) { d.scale[c] = 1.0f / (255.0f * std[c]); d.bias[c] = -mean[c] / std[c]; }
    hipdec_tensor_entry* e = (hipdec_tensor_entry*)calloc((size_t)n, sizeof(hipdec_tensor_entry));
    for (int i = 0; i < n; i++) {
      hipdec_image_info info;
      hipdec_batch_info(prev, i, &info);
      const int side = info.width < info.height ? info.width : info.height;
      e[i].item = i; e[i].left = (info.width - side) / 2; e[i].top = (info.height - side) / 2; e[i].width = e[i].height = side;
    }
    const size_t bytes = hipdec_tensor_bytes(&d, n);
    void* t = bytes ? hipdec_malloc(bytes) : NULL;
    uint16_t* host = (uint16_t*)malloc(bytes ? bytes : 1);
    if (!t || !host || hipdec_batch_to_tensor(prev, &d, e, n, t, bytes, NULL) || hipdec_batch_status(prev) || hipdec_memcpy_d2h(host, t, bytes)) {
      fprintf(stderr, "%s\n", hipdec_last_error());
      return 1;
    }
    unsigned long long sum = 0;
    for (size_t k = 0; k < bytes / 2; k++) sum += host[k];
    printf("tensor %dx3x%dx%d float16, sum of the bit patterns %llu\n", n, tensor, tensor, sum);
    free(host); free(e);
    hipdec_free(t);
  }
  hipdec_batch_free(prev);
  hipdec_shutdown();
  return 0;
}
