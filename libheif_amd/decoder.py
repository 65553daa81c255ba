"""Host-side mirror of the reference's decoder-plugin interface for the HEVC path.

`HipDecoder` follows the call sequence libheif drives through heif_decoder_plugin
(libheif/codecs/decoder.cc:355-563): new_decoder -> push_data (xN) -> decode_next_image -> free,
with the same framing contract as libheif/plugins/decoder_libde265.cc:322-368 and the same error
behaviour (truncated framing -> End_of_data, nothing pushed -> no image).  `Batch` is the grid /
throughput entry point (libheif/image-items/grid.cc:405-453 on the device).  Both are thin ctypes
wrappers over the C ABI in include/heif_hipdec.h — no pixel is computed in Python.
"""
import ctypes as C
import numpy as np
from ._capi import HipDecError, ImageInfo, check, load_library, DeviceBuffer


def _bind(lib):
    if getattr(lib, "_dec_bound", False):
        return lib
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    lib.hipdec_decoder_new.argtypes = [C.POINTER(vp), ci, C.c_uint64]
    lib.hipdec_decoder_free.argtypes = [vp]
    lib.hipdec_decoder_push_data.argtypes = [vp, C.c_char_p, sz]
    lib.hipdec_decoder_decode.argtypes = [vp, C.POINTER(ImageInfo)]
    lib.hipdec_decoder_read_plane.argtypes = [vp, ci, vp, sz]
    lib.hipdec_decoder_coalesce_stats.restype = None
    lib.hipdec_decoder_coalesce_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    lib.hipdec_decoder_chain_stats.restype = None
    lib.hipdec_decoder_chain_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    lib.hipdec_batch_create.argtypes = [C.POINTER(vp), ci, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_uint64]
    lib.hipdec_batch_create_recycling.argtypes = [C.POINTER(vp), ci, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_uint64, vp]
    lib.hipdec_batch_free.argtypes = [vp]
    lib.hipdec_batch_count.argtypes = [vp]
    lib.hipdec_batch_info.argtypes = [vp, ci, C.POINTER(ImageInfo)]
    lib.hipdec_batch_run.argtypes = [vp, vp]
    lib.hipdec_batch_status.argtypes = [vp]
    lib.hipdec_batch_read_plane.argtypes = [vp, ci, ci, vp, sz]
    lib.hipdec_batch_device_plane.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(sz)]
    lib.hipdec_batch_to_rgb.argtypes = [vp, ci, ci, vp, sz, vp]
    lib.hipdec_batch_to_rgb_all.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_batch_run_rgb.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_batch_to_rgb_scaled.argtypes = [vp, ci, ci, ci, ci, ci, vp, sz, vp]
    lib.hipdec_batch_to_rgb_scaled_all.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_batch_read_plane_scaled.argtypes = [vp, ci, ci, ci, ci, ci, vp, sz]
    lib.hipdec_tensor_bytes.restype = sz
    lib.hipdec_tensor_bytes.argtypes = [C.POINTER(TensorDesc), ci]
    lib.hipdec_batch_to_tensor.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), ci, vp, sz, vp]
    lib.hipdec_image_to_tensor.argtypes = [vp, vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), ci, vp, sz, ci]
    lib.hipdec_tensor_stats.restype = None
    lib.hipdec_tensor_stats.argtypes = [C.POINTER(C.c_uint64)] * 2
    lib.hipdec_batch_tensor_block.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(sz)] + [C.POINTER(ci)] * 4
    lib.hipdec_batch_last_timing_us.argtypes = [vp, C.POINTER(C.c_float)]
    lib.hipdec_batch_item_packed_bytes.restype = sz
    lib.hipdec_batch_item_packed_bytes.argtypes = [vp, ci]
    lib.hipdec_batch_pack_item.argtypes = [vp, ci, vp, sz, vp]
    lib.hipdec_copy2d_d2d.argtypes = [vp, sz, vp, sz, sz, sz, vp]
    lib.hipdec_batch_timing_slots.argtypes = [vp, ci]
    lib.hipdec_batch_slot_timing_us.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.hipdec_batch_slot_kernel_timing_us.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.hipdec_batch_read_tap.argtypes = [vp, ci, ci, ci, vp, sz]
    lib.hipdec_batch_read_maps.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, sz]
    lib.hipdec_album_create.argtypes = [C.POINTER(vp), ci, C.POINTER(AlbumPhoto), C.POINTER(C.c_char_p), C.POINTER(sz), ci, C.c_uint64]
    lib.hipdec_album_free.argtypes = [vp]
    lib.hipdec_album_free.restype = None
    lib.hipdec_album_count.argtypes = [vp]
    lib.hipdec_album_info.argtypes = [vp, ci, C.POINTER(ImageInfo)]
    lib.hipdec_album_run.argtypes = [vp, vp]
    lib.hipdec_album_status.argtypes = [vp]
    lib.hipdec_album_canvas_plane.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(sz)]
    lib.hipdec_album_read_plane.argtypes = [vp, ci, ci, vp, sz]
    lib.hipdec_album_to_rgb_all.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_album_to_rgb_scaled_all.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_album_to_tensor.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), ci, vp, sz, vp]
    lib.hipdec_album_stats.restype = None
    lib.hipdec_album_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    lib.hipdec_album_paste_timing_us.argtypes = [vp, C.POINTER(C.c_float)]
    lib.hipdec_orientation_compose.argtypes = [ci, ci, ci]
    lib.hipdec_orientation_from_exif.argtypes = [ci]
    lib.hipdec_batch_to_tensor_oriented.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), ci, vp, sz, vp]
    lib.hipdec_album_to_tensor_oriented.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), ci, vp, sz, vp]
    lib.hipdec_batch_to_rgb_scaled_oriented_all.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_album_to_rgb_scaled_oriented_all.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(vp), C.POINTER(sz), vp]
    lib.hipdec_oriented_stats.restype = None
    lib.hipdec_oriented_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    placed = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(TensorPlace), C.POINTER(TensorFill), vp, ci, vp, sz, vp]
    lib.hipdec_batch_to_tensor_placed.argtypes = placed
    lib.hipdec_album_to_tensor_placed.argtypes = placed
    lib.hipdec_letterbox_place.argtypes = [ci, ci, ci, ci, ci, ci, C.POINTER(TensorPlace)]
    lib.hipdec_placed_stats.restype = None
    lib.hipdec_placed_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    lib.hipdec_batch_to_tensor_framed.argtypes = placed
    lib.hipdec_album_to_tensor_framed.argtypes = placed
    lib.hipdec_resize_crop_place.argtypes = [ci, ci, ci, ci, ci, C.POINTER(TensorPlace)]
    lib.hipdec_framed_stats.restype = None
    lib.hipdec_framed_stats.argtypes = [C.POINTER(C.c_uint64)] * 4
    composed = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(TensorTile), C.POINTER(TensorFill), vp, ci, ci, vp, sz, vp]
    lib.hipdec_batch_to_tensor_composed.argtypes = composed
    lib.hipdec_album_to_tensor_composed.argtypes = composed
    lib.hipdec_compose_visible_area.argtypes = [ci, ci, C.POINTER(TensorTile), ci, ci, C.POINTER(C.c_uint64)]
    lib.hipdec_mosaic_tiles.argtypes = [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(TensorTile)]
    lib.hipdec_sheet_tiles.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, ci, ci, C.POINTER(TensorTile)]
    lib.hipdec_composed_stats.restype = None
    lib.hipdec_composed_stats.argtypes = [C.POINTER(C.c_uint64)] * 5
    packed = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(TensorSample), C.POINTER(TensorPatches), ci, vp, sz, vp]
    lib.hipdec_batch_to_tensor_packed.argtypes = packed
    lib.hipdec_album_to_tensor_packed.argtypes = packed
    lib.hipdec_tensor_packed_layout.argtypes = [C.POINTER(TensorPatches), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                                C.POINTER(C.c_uint64)]
    lib.hipdec_packed_stats.restype = None
    lib.hipdec_packed_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    if hasattr(lib, "hipdec_tensor_warp"):     # (as for the clips below: an older branch's library has no warp stage, and the warped calls say so)
        lib.hipdec_tensor_warp.argtypes = [vp, sz, C.POINTER(WarpDesc), C.POINTER(TensorMap), C.POINTER(TensorFill), C.POINTER(TensorDesc), ci, vp, sz, vp]
        warped = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(WarpDesc), C.POINTER(TensorMap), C.POINTER(TensorFill), ci, vp, sz, vp]
        lib.hipdec_batch_to_tensor_warped.argtypes = warped
        lib.hipdec_album_to_tensor_warped.argtypes = warped
        lib.hipdec_rotate_map.argtypes = [C.c_double, ci, ci, C.POINTER(TensorMap)]
        lib.hipdec_warp_stats.restype = None
        lib.hipdec_warp_stats.argtypes = [C.POINTER(C.c_uint64)] * 2
    if hasattr(lib, "hipdec_tensor_project"):  # (likewise: the projective stage)
        lib.hipdec_tensor_project.argtypes = [vp, sz, C.POINTER(WarpDesc), C.POINTER(TensorProjection), C.POINTER(TensorFill), C.POINTER(TensorDesc), ci, vp, sz, vp]
        projected = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(WarpDesc), C.POINTER(TensorProjection), C.POINTER(TensorFill), ci,
                     vp, sz, vp]
        lib.hipdec_batch_to_tensor_projected.argtypes = projected
        lib.hipdec_album_to_tensor_projected.argtypes = projected
        lib.hipdec_perspective_map.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(TensorProjection)]
        lib.hipdec_quad_map.argtypes = [C.POINTER(C.c_double), ci, ci, C.POINTER(TensorProjection)]
        lib.hipdec_project_stats.restype = None
        lib.hipdec_project_stats.argtypes = [C.POINTER(C.c_uint64)] * 2
    if hasattr(lib, "hipdec_tensor_photo"):    # (likewise: an older branch's library has no photo stage)
        lib.hipdec_tensor_photo.argtypes = [vp, sz, C.POINTER(PhotoDesc), C.POINTER(PhotoChain), C.POINTER(TensorDesc), ci, vp, sz, vp]
        photo = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(PhotoDesc), C.POINTER(PhotoChain), ci, vp, sz, vp]
        lib.hipdec_batch_to_tensor_photo.argtypes = photo
        lib.hipdec_album_to_tensor_photo.argtypes = photo
        lib.hipdec_photo_stats.restype = None
        lib.hipdec_photo_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
    if hasattr(lib, "hipdec_tensor_augment"):  # (likewise: the augment stage)
        lib.hipdec_tensor_augment.argtypes = [vp, sz, C.POINTER(PhotoDesc), C.POINTER(AugmentChain), C.POINTER(TensorDesc), ci, vp, sz, vp]
        augmented = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(PhotoDesc), C.POINTER(AugmentChain), ci, vp, sz, vp]
        lib.hipdec_batch_to_tensor_augmented.argtypes = augmented
        lib.hipdec_album_to_tensor_augmented.argtypes = augmented
        lib.hipdec_augment_stats.restype = None
        lib.hipdec_augment_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
        lib.hipdec_gaussian_box.argtypes = [C.c_double, C.POINTER(ci), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(lib, "hipdec_tensor_recipe"):   # (likewise: the recipe stage)
        lib.hipdec_tensor_recipe.argtypes = [vp, sz, C.POINTER(PhotoDesc), C.POINTER(AugmentChain), C.POINTER(RecipeAffine), ci, C.POINTER(TensorDesc), ci, vp, sz, vp]
        recipe = [vp, C.POINTER(TensorDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(PhotoDesc), C.POINTER(AugmentChain), C.POINTER(RecipeAffine), ci, ci,
                  vp, sz, vp]
        lib.hipdec_batch_to_tensor_recipe.argtypes = recipe
        lib.hipdec_album_to_tensor_recipe.argtypes = recipe
        lib.hipdec_recipe_stats.restype = None
        lib.hipdec_recipe_stats.argtypes = [C.POINTER(C.c_uint64)] * 4
    if hasattr(lib, "hipdec_clips_create"):   # (tools/ab_bench.sh loads an older branch's library through this module: it has no clips, and Clips() says so)
        lib.hipdec_clips_create.argtypes = [C.POINTER(vp), ci, C.POINTER(ci), C.POINTER(C.c_char_p), C.POINTER(sz), C.c_uint64]
        lib.hipdec_clips_free.argtypes = [vp]
        lib.hipdec_clips_free.restype = None
        lib.hipdec_clips_run.argtypes = [vp, vp]
        lib.hipdec_clips_status.argtypes = [vp]
        lib.hipdec_clips_track_count.argtypes = [vp]
        lib.hipdec_clips_frame_count.argtypes = [vp, ci]
        lib.hipdec_clips_frame.argtypes = [vp, ci, ci, C.POINTER(ClipFrame)]
        lib.hipdec_clips_frame_plane.argtypes = [vp, ci, ci, ci, C.POINTER(vp), C.POINTER(sz)]
        lib.hipdec_clips_read_plane.argtypes = [vp, ci, ci, ci, vp, sz]
        lib.hipdec_clips_batch.restype = vp
        lib.hipdec_clips_batch.argtypes = [vp]
        lib.hipdec_clips_stats.restype = None
        lib.hipdec_clips_stats.argtypes = [C.POINTER(C.c_uint64)] * 5
        lib.hipdec_clips_to_tensor.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(ClipDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(ci), ci, vp, sz, vp]
        lib.hipdec_clips_to_tensor_packed.argtypes = [vp, C.POINTER(TensorDesc), C.POINTER(ClipDesc), C.POINTER(TensorEntry), C.POINTER(ci), C.POINTER(ci),
                                                      C.POINTER(TensorSample), C.POINTER(TensorPatches), ci, vp, sz, vp]
        lib.hipdec_clip_packed_layout.argtypes = [C.POINTER(ClipDesc), C.POINTER(TensorPatches), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib._dec_bound = True
    return lib


class AlbumPhoto(C.Structure):
    """hipdec_album_photo"""
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("out_width", C.c_int), ("out_height", C.c_int), ("first_tile", C.c_int), ("reserved", C.c_int)]


class TensorDesc(C.Structure):
    """hipdec_tensor_desc"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class TensorEntry(C.Structure):
    """hipdec_tensor_entry"""
    _fields_ = [("item", C.c_int), ("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("flip", C.c_int)]


class TensorPlace(C.Structure):
    """hipdec_tensor_place"""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class TensorTile(C.Structure):
    """hipdec_tensor_tile"""
    _fields_ = [("canvas", C.c_int), ("place", TensorPlace), ("clip", TensorPlace)]


class TensorFill(C.Structure):
    """hipdec_tensor_fill"""
    _fields_ = [("value", C.c_float * 3), ("domain", C.c_int), ("reserved", C.c_int)]


class TensorSample(C.Structure):
    """hipdec_tensor_sample"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("offset", C.c_uint64)]


class TensorPatches(C.Structure):
    """hipdec_tensor_patches"""
    _fields_ = [("patch", C.c_int), ("merge", C.c_int), ("reserved", C.c_int * 2)]


class TensorMap(C.Structure):
    """hipdec_tensor_map: PIL's AFFINE data, the centre of an output pixel to source coordinates"""
    _fields_ = [("m", C.c_double * 6)]


class WarpDesc(C.Structure):
    """hipdec_warp_desc"""
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("filter", C.c_int), ("reserved", C.c_int)]


class TensorProjection(C.Structure):
    """hipdec_tensor_projection: PIL's PERSPECTIVE data, or the eight coefficients of its QUAD method, and the kind"""
    _fields_ = [("a", C.c_double * 8), ("kind", C.c_int), ("reserved", C.c_int)]


class PhotoOp(C.Structure):
    """hipdec_photo_op"""
    _fields_ = [("op", C.c_int), ("reserved", C.c_int), ("value", C.c_double)]


class PhotoChain(C.Structure):
    """hipdec_photo_chain: up to PHOTO_MAX_OPS operations, applied in order"""
    _fields_ = [("n_ops", C.c_int), ("reserved", C.c_int), ("ops", PhotoOp * 4)]


class PhotoDesc(C.Structure):
    """hipdec_photo_desc"""
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("reserved", C.c_int * 2)]


class AugmentChain(C.Structure):
    """hipdec_augment_chain: up to AUGMENT_MAX_OPS operations, applied in order"""
    _fields_ = [("n_ops", C.c_int), ("reserved", C.c_int), ("ops", PhotoOp * 8)]


class RecipeAffine(C.Structure):
    """hipdec_recipe_affine: the map, the warp filter and Pillow's fillcolor of one affine step of a recipe chain"""
    _fields_ = [("map", TensorMap), ("filter", C.c_int), ("fill", C.c_int * 3)]


class ClipFrame(C.Structure):
    """hipdec_clip_frame"""
    _fields_ = [("item", C.c_int), ("sample", C.c_int), ("poc", C.c_int), ("sequence", C.c_int), ("info", ImageInfo)]


class ClipDesc(C.Structure):
    """hipdec_clip_desc"""
    _fields_ = [("frames", C.c_int), ("order", C.c_int), ("temporal_patch", C.c_int), ("reserved", C.c_int)]


CLIP_ORDERS = {"TCHW": (0, "NCHW"), "THWC": (0, "NHWC"), "CTHW": (1, "NCHW")}   # (hipdec_clip_order, layout of a frame)
FILL_DOMAINS = {"component": 0, "element": 1}                                # hipdec_fill_domain
TENSOR_DTYPES = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3}       # hipdec_tensor_dtype
TENSOR_LAYOUTS = {"NCHW": 0, "NHWC": 1}                                       # hipdec_tensor_layout
_TENSOR_NUMPY = {"uint8": np.uint8, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}   # (NumPy has no bfloat16: its bits)


def tensor_scale_bias(mean=None, std=None, scale=None, bias=None, max_value=255):
    """The per-channel (scale, bias) of a tensor description, float32 arrays of three.  Either scale / bias as they are (a number or three; defaults
    1 and 0: the raw component values), or the usual 0..1 convention of mean / std, (V / max_value - mean) / std, folded in float32 arithmetic as
        scale[c] = float32(1) / (float32(max_value) * float32(std[c]))        bias[c] = -float32(mean[c]) / float32(std[c])
    (mean defaults to 0, std to 1).  max_value is the largest component value V: 255, or 2^bits - 1 for float dtypes from sources above 8 bits."""
    three = lambda v, d: np.broadcast_to(np.asarray(d if v is None else v, np.float32), (3,)).copy()
    if mean is not None or std is not None:
        if scale is not None or bias is not None:
            raise ValueError("give mean / std or scale / bias, not both")
        m, sd = three(mean, 0.0), three(std, 1.0)
        return np.float32(1) / (np.float32(max_value) * sd), -m / sd
    return three(scale, 1.0), three(bias, 0.0)


def tensor_desc(size, dtype="float16", layout="NCHW", filter=1, scale=None, bias=None):
    """hipdec_tensor_desc for size = (width, height)"""
    if dtype not in TENSOR_DTYPES:
        raise ValueError("dtype must be one of %s" % sorted(TENSOR_DTYPES))
    if layout not in TENSOR_LAYOUTS:
        raise ValueError("layout must be NCHW or NHWC")
    d = TensorDesc()
    d.width, d.height, d.dtype, d.layout, d.filter = int(size[0]), int(size[1]), TENSOR_DTYPES[dtype], TENSOR_LAYOUTS[layout], int(filter)
    sc, bi = tensor_scale_bias(scale=scale, bias=bias)
    for c in range(3):
        d.scale[c], d.bias[c] = float(sc[c]), float(bi[c])
    return d


def tensor_entries(entries):
    """a ctypes array of hipdec_tensor_entry from (item, left, top, width, height[, flip]) tuples or TensorEntry objects"""
    arr = (TensorEntry * len(entries))()
    for k, e in enumerate(entries):
        if isinstance(e, TensorEntry):
            arr[k] = e
        else:
            e = tuple(int(v) for v in e)
            arr[k] = TensorEntry(*(e + (0,) * (6 - len(e))))
    return arr


def tensor_shape(n, size, layout):
    return (n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3)


def center_crop_entry(item, width, height, crop_width, crop_height=None, flip=False):
    """the window of crop_width x crop_height (default: square) in the middle of a width x height picture, as an entry tuple; the offsets round down"""
    cw = int(crop_width)
    ch = cw if crop_height is None else int(crop_height)
    if cw < 1 or ch < 1 or cw > width or ch > height:
        raise ValueError("a crop of %d x %d does not fit a picture of %d x %d" % (cw, ch, width, height))
    return (int(item), (width - cw) // 2, (height - ch) // 2, cw, ch, int(bool(flip)))


def random_resized_crop_entries(rng, sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_probability=0.5, items=None, attempts=10):
    """One random-resized-crop window per picture, as entry tuples: `sizes` are the pictures' (width, height), `items` the batch items they name
    (default 0, 1, ...).  The usual recipe in plain host arithmetic, deterministic for a seeded numpy.random.Generator: up to `attempts` draws of an area
    fraction uniform in `scale` and an aspect ratio log-uniform in `ratio`, w = round(sqrt(area * r)), h = round(sqrt(area / r)), taken when it fits, at an
    offset uniform over the positions that fit; failing that, the largest centred window whose aspect ratio is clamped into `ratio`.  Then one draw for the
    flip.  Every picture consumes the generator in this order, whether a draw fits or not."""
    out = []
    for k, (w, h) in enumerate(sizes):
        item = k if items is None else int(items[k])
        area = float(w) * float(h)
        win = None
        for _ in range(attempts):
            a = area * rng.uniform(scale[0], scale[1])
            r = float(np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1]))))
            cw, ch = int(round(np.sqrt(a * r))), int(round(np.sqrt(a / r)))
            if win is None and 0 < cw <= w and 0 < ch <= h:
                left, top = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
                win = (left, top, cw, ch)
        if win is None:
            r = min(max(w / h, ratio[0]), ratio[1])
            cw, ch = (w, max(1, min(h, int(round(w / r))))) if w / h <= r else (max(1, min(w, int(round(h * r)))), h)
            win = ((w - cw) // 2, (h - ch) // 2, cw, ch)
        out.append((item,) + win + (int(rng.random() < flip_probability),))
    return out


def tensor_stats():
    """(tensors written by Batch.to_tensor / color.image_to_tensor, their entries) since the library was loaded"""
    lib = _bind(load_library())
    a, b = C.c_uint64(), C.c_uint64()
    lib.hipdec_tensor_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def _torch_gpu():
    """torch when it is importable and sees a GPU, else None"""
    try:
        import torch
    except Exception:
        return None
    return torch if torch.cuda.is_available() else None


def _info_dict(info):
    return {f: getattr(info, f) for f, _ in ImageInfo._fields_}


def coalesce_stats():
    """(decode requests, launch sets, requests that shared a launch set) since the library was loaded"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_decoder_coalesce_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def chain_stats():
    """(look-ahead chains of sequence tracks, launch sets issued for them, launch sets that held several tracks' chains) since the library was loaded"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_decoder_chain_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def set_sequence_pipeline(chains):
    """look-ahead chains of one track in flight at a time (hipdec_set_sequence_pipeline; 1: every chain is waited for where it is launched)"""
    lib = load_library()
    lib.hipdec_set_sequence_pipeline.argtypes = [C.c_int]
    lib.hipdec_set_sequence_pipeline.restype = None
    lib.hipdec_set_sequence_pipeline(int(chains))


def pipeline_stats():
    """(chains that were left in flight when they were enqueued, roll-backs of failed ones) since the library was loaded"""
    lib = load_library()
    lib.hipdec_decoder_pipeline_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.hipdec_decoder_pipeline_stats.restype = None
    a, b = C.c_uint64(), C.c_uint64()
    lib.hipdec_decoder_pipeline_stats(C.byref(a), C.byref(b))
    return a.value, b.value


SCALE_NEAREST, SCALE_BOX = 0, 1   # hipdec_scale_filter
SCALE_BILINEAR, SCALE_BICUBIC = 16, 17   # ... PIL.Image.resize(BILINEAR / BICUBIC) bit for bit (to_tensor, to_rgb_scaled*; not planes_scaled)


def resample_taps(in_size, out_size, filter, out_index):
    """(first input sample, [coefficients with 22 fractional bits]) of output sample out_index along an axis of in_size -> out_size samples, as the
    SCALE_BILINEAR / SCALE_BICUBIC kernel receives them (hipdec_resample_taps; host only)"""
    lib = load_library()
    lib.hipdec_resample_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]
    lib.hipdec_resample_taps.restype = C.c_int
    first = C.c_int()
    n = lib.hipdec_resample_taps(in_size, out_size, filter, out_index, C.byref(first), None, 0)
    if n < 0:
        raise ValueError("resample_taps(%r, %r, %r, %r)" % (in_size, out_size, filter, out_index))
    k = (C.c_int32 * max(n, 1))()
    check(min(lib.hipdec_resample_taps(in_size, out_size, filter, out_index, C.byref(first), k, n), 0))
    return first.value, list(k[:n])


# hipdec_orientation: code = r + 4 * m - the stored picture rotated counter-clockwise by r quarter turns, then mirrored horizontally if m
ORIENT_0, ORIENT_CCW90, ORIENT_180, ORIENT_CCW270 = 0, 1, 2, 3
ORIENT_MIRROR, ORIENT_CCW90_MIRROR, ORIENT_180_MIRROR, ORIENT_CCW270_MIRROR = 4, 5, 6, 7
XF_ROTATE_CCW, XF_MIRROR = 0, 1                                                # hipdec_transform_op


def orientation_compose(orientation, op, arg):
    """the code of "apply op (XF_ROTATE_CCW with 90 / 180 / 270, XF_MIRROR with 0 vertical / 1 horizontal) to the displayed picture of `orientation`"
    (hipdec_orientation_compose; host only): folds an item's 'irot' / 'imir' list, in 'ipma' order, into one code"""
    code = _bind(load_library()).hipdec_orientation_compose(orientation, op, arg)
    if code < 0:
        raise ValueError("orientation_compose(%r, %r, %r)" % (orientation, op, arg))
    return code


def orientation_from_exif(exif):
    """the code of EXIF orientation 1 .. 8 (hipdec_orientation_from_exif; host only)"""
    code = _bind(load_library()).hipdec_orientation_from_exif(exif)
    if code < 0:
        raise ValueError("EXIF orientation %r is not 1 .. 8" % (exif,))
    return code


def oriented_size(code, width, height):
    """the displayed size of a stored picture of width x height"""
    return (height, width) if code & 1 else (width, height)


def stored_window(code, stored_width, stored_height, left, top, width, height):
    """A window given in DISPLAYED coordinates (left, top, width, height inside the displayed picture of a stored_width x stored_height picture with
    orientation `code`) as the (left, top, width, height) in the stored picture that a tensor entry needs: the oriented result of that entry shows
    exactly the displayed window."""
    dw, dh = oriented_size(code, stored_width, stored_height)
    if width < 1 or height < 1 or left < 0 or top < 0 or left + width > dw or top + height > dh:
        raise ValueError("window %d x %d at (%d, %d) leaves the displayed picture of %d x %d" % (width, height, left, top, dw, dh))
    r, m = code & 3, code >> 2
    if m:                                   # undo the mirror of the displayed picture
        left = dw - left - width
    # undo r quarter turns counter-clockwise, one at a time: out(X, Y) = in(w - 1 - Y, X) on a w x h picture that becomes h x w
    w, h = dw, dh
    for _ in range(r):
        left, top, width, height = h - top - height, left, height, width
        w, h = h, w
    return left, top, width, height


def oriented_stats():
    """(launches of the oriented kernels, entries they wrote, entries with a quarter turn) since load"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_oriented_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _orientation_array(orientations, n):
    codes = [int(c) for c in orientations]
    if len(codes) != n:
        raise ValueError("%d orientations for %d entries" % (len(codes), n))
    return (C.c_int * n)(*codes)


def tensor_places(places, n=None):
    """a ctypes array of hipdec_tensor_place from (x, y, width, height) tuples or TensorPlace objects"""
    places = list(places)
    if n is not None and len(places) != n:
        raise ValueError("%d places for %d entries" % (len(places), n))
    arr = (TensorPlace * len(places))()
    for k, p in enumerate(places):
        arr[k] = p if isinstance(p, TensorPlace) else TensorPlace(*(int(v) for v in p))
    return arr


def tensor_fill(fill, fill_domain="component"):
    """hipdec_tensor_fill from a number or three per channel; fill_domain "component" (a pixel's component value, normalised as pixels are) or "element"
    (the tensor element itself)"""
    if fill_domain not in FILL_DOMAINS:
        raise ValueError("fill_domain must be 'component' or 'element'")
    f = TensorFill()
    v = np.broadcast_to(np.asarray(fill, np.float32), (3,))
    for c in range(3):
        f.value[c] = float(v[c])
    f.domain = FILL_DOMAINS[fill_domain]
    return f


_ANCHORS = {"topleft": 0, "center": 1}


def letterbox_place(src_size, canvas_size, upscale=True, anchor="center"):
    """(x, y, width, height): the rectangle of a displayed sample of src_size = (width, height) fitted into canvas_size = (width, height) with its aspect
    ratio kept (hipdec_letterbox_place; host only).  upscale False: a source that fits both ways keeps its size.  anchor "center" or "topleft"."""
    if anchor not in _ANCHORS:
        raise ValueError("anchor must be 'center' or 'topleft'")
    pl = TensorPlace()
    if _bind(load_library()).hipdec_letterbox_place(int(src_size[0]), int(src_size[1]), int(canvas_size[0]), int(canvas_size[1]), int(bool(upscale)), _ANCHORS[anchor],
                                                     C.byref(pl)) != 0:
        raise ValueError("letterbox_place(%r, %r)" % (tuple(src_size), tuple(canvas_size)))
    return pl.x, pl.y, pl.width, pl.height


def letterbox_places(sizes, canvas_size, upscale=True, anchor="center"):
    """letterbox_place for a list of DISPLAYED sizes (oriented_size() of the stored ones): the `places` of a to_tensor call"""
    return [letterbox_place(s, canvas_size, upscale, anchor) for s in sizes]


def placed_stats():
    """(placed to_tensor calls, their entries, launches of the margin kernel) since load"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_placed_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def resize_crop_place(src_size, resize, crop):
    """(x, y, width, height): torchvision's Resize(resize) -> CenterCrop(crop) on a DISPLAYED sample of src_size = (width, height), as the rectangle of a
    to_tensor(frames=) call whose canvas is crop = (width, height) (hipdec_resize_crop_place; host only).  The shorter side becomes `resize`, the longer
    floor(resize * long / short); the offsets are negative where the resized sample is larger than the crop."""
    pl = TensorPlace()
    if _bind(load_library()).hipdec_resize_crop_place(int(src_size[0]), int(src_size[1]), int(resize), int(crop[0]), int(crop[1]), C.byref(pl)) != 0:
        raise ValueError("resize_crop_place(%r, %r, %r)" % (tuple(src_size), resize, tuple(crop)))
    return pl.x, pl.y, pl.width, pl.height


def resize_crop_places(sizes, resize, crop):
    """resize_crop_place for a list of DISPLAYED sizes (oriented_size() of the stored ones): the `frames` of a to_tensor call"""
    return [resize_crop_place(s, resize, crop) for s in sizes]


def random_crop_places(rng, sizes, crop, padding=0, pad_if_needed=False):
    """the `frames` of torchvision's RandomCrop(crop, padding, pad_if_needed) for samples of the DISPLAYED sizes (width, height), crop = (width, height): the
    sample keeps its size, is padded by `padding` - a number, (left / right, top / bottom) or (left, top, right, bottom) - and, with pad_if_needed, by
    crop - side on both sides of an axis that is still shorter than the crop; the crop's corner is drawn uniformly from the padded picture with
    rng.integers (a numpy Generator), x before y, sample by sample.  A padded picture smaller than the crop raises ValueError."""
    pad = (padding,) * 4 if np.isscalar(padding) else tuple(int(v) for v in padding)
    if len(pad) == 2:
        pad = (pad[0], pad[1], pad[0], pad[1])
    if len(pad) != 4 or min(pad) < 0:
        raise ValueError("padding must be a non-negative number, a pair or four of them")
    cw, ch = int(crop[0]), int(crop[1])
    out = []
    for w, h in sizes:
        w, h = int(w), int(h)
        left, top, pw, ph = pad[0], pad[1], w + pad[0] + pad[2], h + pad[1] + pad[3]
        if pad_if_needed and pw < cw:
            left, pw = left + cw - pw, pw + 2 * (cw - pw)
        if pad_if_needed and ph < ch:
            top, ph = top + ch - ph, ph + 2 * (ch - ph)
        if pw < cw or ph < ch:
            raise ValueError("the padded sample of %d x %d is smaller than the crop of %d x %d" % (pw, ph, cw, ch))
        i = int(rng.integers(0, pw - cw + 1))
        j = int(rng.integers(0, ph - ch + 1))
        out.append((left - i, top - j, w, h))
    return out


def framed_stats():
    """(framed to_tensor calls, their entries, pieces of work that held a visible pixel, pieces skipped) since load (hipdec_framed_stats)"""
    lib = _bind(load_library())
    v = [C.c_uint64() for _ in range(4)]
    lib.hipdec_framed_stats(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def tensor_tiles(tiles, n=None):
    """a ctypes array of hipdec_tensor_tile from (canvas, place, clip) tuples - place and clip (x, y, width, height), clip None or (0, 0, 0, 0) for the whole
    canvas - or TensorTile objects"""
    tiles = list(tiles)
    if n is not None and len(tiles) != n:
        raise ValueError("%d tiles for %d entries" % (len(tiles), n))
    arr = (TensorTile * len(tiles))()
    for k, t in enumerate(tiles):
        if isinstance(t, TensorTile):
            arr[k] = t
            continue
        canvas, place, clip = t
        arr[k] = TensorTile(int(canvas), TensorPlace(*(int(v) for v in place)), TensorPlace(*(int(v) for v in (clip if clip is not None else (0, 0, 0, 0)))))
    return arr


def _tiles_out(arr):
    return [(t.canvas, (t.place.x, t.place.y, t.place.width, t.place.height), (t.clip.x, t.clip.y, t.clip.width, t.clip.height)) for t in arr]


def mosaic_tiles(canvas_size, center, sizes, canvas=0):
    """the four (canvas, place, clip) tiles of YOLOv5's mosaic-4 (hipdec_mosaic_tiles; host only): four DISPLAYED, already resized samples of
    sizes[k] = (width, height) around center = (xc, yc) on a canvas of canvas_size = (width, height) - sample 0 above left of the centre, 1 above right,
    2 below left, 3 below right, each clipped to its quadrant.  The `tiles` of a to_tensor_composed call (fill=114 is the usual grey)."""
    sizes = [(int(w), int(h)) for w, h in sizes]
    if len(sizes) != 4:
        raise ValueError("mosaic_tiles takes four sizes")
    out = (TensorTile * 4)()
    if _bind(load_library()).hipdec_mosaic_tiles(int(canvas_size[0]), int(canvas_size[1]), int(center[0]), int(center[1]), (C.c_int * 4)(*[s[0] for s in sizes]),
                                                 (C.c_int * 4)(*[s[1] for s in sizes]), int(canvas), out) != 0:
        raise ValueError("mosaic_tiles(%r, %r, %r)" % (tuple(canvas_size), tuple(center), sizes))
    return _tiles_out(out)


def sheet_tiles(grid, cell, sizes, gap=0, upscale=True, canvas=0):
    """the (canvas, place, clip) tiles of a contact sheet (hipdec_sheet_tiles; host only): grid = (cols, rows) cells of cell = (width, height) with `gap`
    pixels between them, the DISPLAYED sample k of sizes[k] = (width, height) letterboxed (centred) into cell k, row-major, and clipped to it.  The canvas of
    the to_tensor_composed call is sheet_size(grid, cell, gap)."""
    sizes = [(int(w), int(h)) for w, h in sizes]
    n = len(sizes)
    out = (TensorTile * max(n, 1))()
    if _bind(load_library()).hipdec_sheet_tiles(int(grid[0]), int(grid[1]), int(cell[0]), int(cell[1]), int(gap), (C.c_int * max(n, 1))(*[s[0] for s in sizes]),
                                                (C.c_int * max(n, 1))(*[s[1] for s in sizes]), n, int(bool(upscale)), int(canvas), out) != 0:
        raise ValueError("sheet_tiles(%r, %r, %d sizes, gap %r)" % (tuple(grid), tuple(cell), n, gap))
    return _tiles_out(out)[:n]


def sheet_size(grid, cell, gap=0):
    """(width, height) of the sheet sheet_tiles lays out"""
    return grid[0] * cell[0] + (grid[0] - 1) * gap, grid[1] * cell[1] + (grid[1] - 1) * gap


def cutmix_tiles(size, boxes):
    """CutMix over len(boxes) canvases of size = (width, height): (tiles, order) with two tiles per canvas - the base sample whole-canvas, then its partner
    at the canvas' size clipped to boxes[k] = (x, y, width, height) - and order[e] = (canvas, role), role 0 the base and 1 the partner: the entry list the
    tiles imply is the base's entry followed by the partner's, canvas by canvas.  compose_visible_area(size, tiles)[2 * k] / (width * height) is lambda."""
    w, h = int(size[0]), int(size[1])
    tiles, order = [], []
    for k, box in enumerate(boxes):
        tiles += [(k, (0, 0, w, h), (0, 0, 0, 0)), (k, (0, 0, w, h), tuple(int(v) for v in box))]
        order += [(k, 0), (k, 1)]
    return tiles, order


def compose_visible_area(size, tiles, n_canvases=None):
    """the pixels every entry of a to_tensor_composed call owns on canvases of size = (width, height) (hipdec_compose_visible_area; host only)"""
    arr = tensor_tiles(tiles)
    n = len(arr)
    nc = (max(t.canvas for t in arr) + 1 if n else 0) if n_canvases is None else int(n_canvases)
    area = (C.c_uint64 * max(n, 1))()
    if _bind(load_library()).hipdec_compose_visible_area(int(size[0]), int(size[1]), arr, n, nc, area) != 0:
        raise ValueError("compose_visible_area: %s" % _bind(load_library()).hipdec_last_error().decode())
    return [int(a) for a in area[:n]]


def composed_stats():
    """(composed to_tensor calls, their entries, pieces recorded, fully hidden entries, launches of the cover kernel) since load (hipdec_composed_stats)"""
    lib = _bind(load_library())
    v = [C.c_uint64() for _ in range(5)]
    lib.hipdec_composed_stats(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def _to_tensor_composed(self, lib_call, size, tiles, entries, n_canvases, orientations, fill, fill_domain, mask, filter, dtype, layout, mean, std, scale, bias, out,
                        stream):
    n = self.n if entries is None else len(entries)
    tarr = tensor_tiles(tiles, n)
    nc = (max(t.canvas for t in tarr) + 1 if n else 0) if n_canvases is None else int(n_canvases)
    call = lambda h, desc, arr, codes, _places, f, mask_ptr, n, ptr, room, stream: lib_call(h, desc, arr, codes, tarr, f, mask_ptr, n, nc, ptr, room, stream)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations, (None, fill, fill_domain, mask), canvases=nc)


def packed_layout(sizes, patch=0, merge=1):
    """(offsets, tokens, total elements) of samples of the DISPLAYED sizes (width, height) packed back to back in entry order
    (hipdec_tensor_packed_layout; host only): offsets[e] is the index of sample e's first element, tokens[e] its (width / patch) * (height / patch) patch
    tokens (0 for dense samples, patch 0).  A size that is no multiple of patch * merge raises ValueError."""
    lib = _bind(load_library())
    n = len(sizes)
    ws, hs = (C.c_int * n)(*(int(s[0]) for s in sizes)), (C.c_int * n)(*(int(s[1]) for s in sizes))
    offs, toks, total = (C.c_uint64 * n)(), (C.c_uint32 * n)(), C.c_uint64()
    pt = TensorPatches(int(patch), int(merge))
    if lib.hipdec_tensor_packed_layout(C.byref(pt), ws, hs, n, offs, toks, C.byref(total)) != 0:
        raise ValueError("packed_layout: %s" % lib.hipdec_last_error().decode())
    return list(offs), list(toks), total.value


def packed_stats():
    """(packed to_tensor calls, their entries, entries written as patch sequences) since load"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_packed_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _to_tensor_packed(self, call, sizes, entries, patch, merge, dtype, layout, mean, std, scale, bias, filter, orientations, offsets, out, stream):
    """Batch.to_tensor_packed / Album.to_tensor_packed: the samples, the 1-D output buffer (DeviceBuffer or torch.Tensor) and the stream, then `call`"""
    n = self.n if entries is None else len(entries)
    sizes = [(int(w), int(h)) for w, h in sizes]
    if len(sizes) != n:
        raise ValueError("%d sizes for %d entries" % (len(sizes), n))
    patch, merge = int(patch), int(merge)
    if offsets is None:
        offsets, _, total = packed_layout(sizes, patch, merge)
    else:
        offsets = [int(o) for o in offsets]
        if len(offsets) != n:
            raise ValueError("%d offsets for %d entries" % (len(offsets), n))
        total = max(o + 3 * w * h for o, (w, h) in zip(offsets, sizes))
    samples = (TensorSample * n)(*(TensorSample(w, h, o) for (w, h), o in zip(sizes, offsets)))
    pt = TensorPatches(patch, merge)
    codes = None if orientations is None else _orientation_array(orientations, n)
    d0 = self.info(0)
    max_value = (1 << d0["bit_depth_luma"]) - 1 if (dtype != "uint8" and d0["bit_depth_luma"] > 8) else 255
    sc, bi = tensor_scale_bias(mean, std, scale, bias, max_value)
    desc = tensor_desc((0, 0), dtype, layout, filter, sc, bi)
    item = np.dtype(_TENSOR_NUMPY[dtype]).itemsize
    arr = None if entries is None else tensor_entries(entries)
    host_wait = False
    if out is None:
        torch = _torch_gpu()
        out = torch.empty((total,), dtype=getattr(torch, dtype), device="cuda") if torch is not None else DeviceBuffer(max(total * item, 1))
    if isinstance(out, DeviceBuffer):
        ptr, room = out.ptr, out.nbytes
    else:
        import torch
        if not isinstance(out, torch.Tensor) or not out.is_cuda:
            raise TypeError("out must be a DeviceBuffer or a CUDA / HIP torch.Tensor")
        if out.dim() != 1 or not out.is_contiguous():
            raise ValueError("out must be a contiguous 1-D tensor")
        if out.dtype != getattr(torch, dtype):
            raise ValueError("out has dtype %s, the tensor has %s" % (out.dtype, dtype))
        ptr, room = out.data_ptr(), out.numel() * item
        if stream is None:
            ts = torch.cuda.current_stream(out.device)
            stream = ts.cuda_stream or None
            if stream is None:   # (torch's legacy default stream: ordered on the host, as in to_tensor)
                ts.synchronize()
                host_wait = True
    check(call(self._h, C.byref(desc), arr, codes, samples, C.byref(pt), n, ptr, room, stream))
    if host_wait:
        check(self._lib.hipdec_stream_synchronize(None))
    self._tensor_packed = (out, room // item, _TENSOR_NUMPY[dtype], stream, sizes, offsets, patch, layout)
    grids = [(h // patch, w // patch) for w, h in sizes] if patch else None
    return out, offsets, grids


def _tensor_packed_to_host(self):
    """the last to_tensor_packed() result on the host; waits for its stream.  Patch sequences: one array [tokens, 3 * patch * patch], the samples' tokens in
    entry order (gaps between samples left out).  Dense samples: (flat, view) - the whole output as a flat array, and view(e), sample e of it in the shape
    of its layout, (3, height, width) or (height, width, 3).  bfloat16 comes as uint16 bit patterns."""
    out, elems, dt, stream, sizes, offsets, patch, layout = self._tensor_packed
    check(self._lib.hipdec_stream_synchronize(stream))
    if isinstance(out, DeviceBuffer):
        flat = out.to_numpy((elems,), dt)
    else:
        import torch
        t = out.view(torch.int16) if dt == np.uint16 else out
        flat = t.cpu().numpy()
        flat = flat.view(np.uint16) if dt == np.uint16 else flat
    if patch:
        return np.concatenate([flat[o:o + 3 * w * h] for o, (w, h) in zip(offsets, sizes)]).reshape(-1, 3 * patch * patch)

    def view(e):
        w, h = sizes[e]
        return flat[offsets[e]:offsets[e] + 3 * w * h].reshape((3, h, w) if layout == "NCHW" else (h, w, 3))
    return flat, view


def tensor_maps(maps, n=None):
    """a ctypes array of hipdec_tensor_map from sequences of six numbers (PIL's AFFINE data) or TensorMap objects"""
    maps = list(maps)
    if n is not None and len(maps) != n:
        raise ValueError("%d maps for %d entries" % (len(maps), n))
    arr = (TensorMap * max(len(maps), 1))()
    for k, m in enumerate(maps):
        if isinstance(m, TensorMap):
            arr[k] = m
        else:
            m = [float(v) for v in m]
            if len(m) != 6:
                raise ValueError("a map has six coefficients, not %d" % len(m))
            arr[k] = TensorMap((C.c_double * 6)(*m))
    return arr


def warp_desc(src_size, warp_filter=SCALE_BILINEAR):
    """hipdec_warp_desc for src_size = (width, height) of the intermediate picture"""
    return WarpDesc(int(src_size[0]), int(src_size[1]), int(warp_filter), 0)


def warp_stats():
    """(launches of the warp kernel - one per warped call that wrote anything -, the entries they wrote) since load"""
    lib = _bind(load_library())
    a, b = C.c_uint64(), C.c_uint64()
    lib.hipdec_warp_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def rotate_matrix(angle, size):
    """The six coefficients PIL.Image.rotate(angle) - counter-clockwise degrees about the centre, without expand or translate - hands to its AFFINE
    transform for a picture of size = (width, height), computed as Pillow computes them: the angle taken mod 360, cos and sin of -radians(angle) rounded with
    round(., 15), the centre (width / 2, height / 2), and the translation as the matrix applied to minus the centre, plus the centre.  (Image.rotate
    short-cuts multiples of 90 degrees on square pictures to transposes; the map given here produces the same pixels.)"""
    import math
    w, h = size
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = transform(-cx, -cy)
    m[2] += cx
    m[5] += cy
    return tuple(m)


def affine_matrix(center, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0)):
    """The six coefficients of the INVERSE, in float64, of  T(center + translate) . R(angle) . scale . Shear(shear) . T(-center)  - the map from output to
    source coordinates that a forward transform "rotate by `angle` degrees (counter-clockwise on the screen), scale, shear by (sx, sy) degrees about `center`,
    then move by `translate`" needs, for RandomAffine-style parameters.  R(angle) = [[cos, sin], [-sin, cos]] of radians(angle) in image coordinates (y down);
    Shear = [[1, -tan(sx)], [0, 1]] applied after [[1, 0], [-tan(sy), 1]].  The 2 x 2 part is inverted in closed form.
    NOT pinned to torchvision's _get_inverse_affine_matrix: torchvision is not installed where this library is tested, so the conventions above are this
    function's own; with shear (0, 0) the result for `angle` is rotate_matrix(angle) up to the rounding Pillow applies to cos and sin."""
    import math
    cx, cy = float(center[0]), float(center[1])
    tx, ty = float(translate[0]), float(translate[1])
    sx, sy = math.radians(float(shear[0])), math.radians(float(shear[1]))
    r = math.radians(float(angle))
    c, s_ = math.cos(r), math.sin(r)
    # Shear = [[1, -tan sx], [0, 1]] . [[1, 0], [-tan sy, 1]]
    h00, h01, h10, h11 = 1.0 + math.tan(sx) * math.tan(sy), -math.tan(sx), -math.tan(sy), 1.0
    k = float(scale)
    f00, f01 = k * (c * h00 + s_ * h10), k * (c * h01 + s_ * h11)
    f10, f11 = k * (-s_ * h00 + c * h10), k * (-s_ * h01 + c * h11)
    det = f00 * f11 - f01 * f10
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("affine_matrix: the transform is singular")
    i00, i01, i10, i11 = f11 / det, -f01 / det, -f10 / det, f00 / det
    # forward: p' = F (p - center) + center + translate;  inverse: p = I (p' - center - translate) + center
    ox, oy = cx + tx, cy + ty
    return (i00, i01, cx - (i00 * ox + i01 * oy), i10, i11, cy - (i10 * ox + i11 * oy))


def _warped_call(lib_call, n, size, src_size, maps, warp_filter, fill, fill_domain, orientations):
    """the argument adapter of the warped entry points for _to_tensor"""
    wd = warp_desc(size if src_size is None else src_size, warp_filter)
    marr = tensor_maps(maps, n)
    f = None if fill is None else tensor_fill(fill, fill_domain)
    codes = None if orientations is None else _orientation_array(orientations, n)
    keep = (wd, marr, f, codes)
    return lambda h, desc, arr, n_, ptr, room, stream: lib_call(h, desc, arr, codes, C.byref(wd), marr, f, n_, ptr, room, stream), keep


def _to_tensor_warped(self, lib_call, size, maps, entries, src_size, warp_filter, fill, fill_domain, orientations, filter, dtype, layout, mean, std, scale,
                      bias, out, stream):
    n = self.n if entries is None else len(entries)
    call, _keep = _warped_call(lib_call, n, size, src_size, maps, warp_filter, fill, fill_domain, orientations)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)


# the projective stage (hipdec_tensor_project): PIL.Image.transform(size, PERSPECTIVE | QUAD, ...) on the 8-bit picture, bit for bit
PROJECT_PERSPECTIVE, PROJECT_QUAD = 0, 1
PROJECT_KINDS = {"perspective": PROJECT_PERSPECTIVE, "quad": PROJECT_QUAD}


def tensor_projections(maps, n=None):
    """a ctypes array of hipdec_tensor_projection.  A map is a sequence of eight numbers - PIL's PERSPECTIVE data -, a (kind, eight numbers) pair with kind
    PROJECT_PERSPECTIVE / PROJECT_QUAD or "perspective" / "quad" (QUAD: the coefficients quad_map() makes, not the corners), or a TensorProjection"""
    maps = list(maps)
    if n is not None and len(maps) != n:
        raise ValueError("%d maps for %d entries" % (len(maps), n))
    arr = (TensorProjection * max(len(maps), 1))()
    for k, m in enumerate(maps):
        if isinstance(m, TensorProjection):
            arr[k] = m
            continue
        m = tuple(m)
        kind = PROJECT_PERSPECTIVE
        if len(m) == 2:
            kind, m = m
            if isinstance(kind, str):
                if kind.lower() not in PROJECT_KINDS:
                    raise ValueError("unknown kind of map %r" % (kind,))
                kind = PROJECT_KINDS[kind.lower()]
        a = [float(v) for v in m]
        if len(a) != 8:
            raise ValueError("a projective map has eight coefficients, not %d" % len(a))
        arr[k] = TensorProjection((C.c_double * 8)(*a), int(kind), 0)
    return arr


def perspective_map(startpoints, endpoints):
    """The TensorProjection (PERSPECTIVE) that reads output point endpoints[k] from source point startpoints[k], k = 0 .. 3, each an (x, y) pair - the
    library's statement of torchvision's _get_perspective_coeffs(startpoints, endpoints), computed by the C helper hipdec_perspective_map (an 8 x 8 system
    in float64, Gaussian elimination with partial pivoting).  NOT pinned to torchvision, which is not installed where this library is tested.  Four
    collinear or repeated points raise HipDecError."""
    lib = _bind(load_library())
    sp = [float(v) for p in startpoints for v in p]
    ep = [float(v) for p in endpoints for v in p]
    if len(sp) != 8 or len(ep) != 8:
        raise ValueError("perspective_map takes four (x, y) start points and four end points")
    out = TensorProjection()
    check(lib.hipdec_perspective_map((C.c_double * 8)(*sp), (C.c_double * 8)(*ep), C.byref(out)))
    return out


def quad_map(corners, size):
    """The TensorProjection (QUAD) of PIL.Image.transform(size, QUAD, corners): corners = (nw, sw, se, ne), each an (x, y) pair in source coordinates - or the
    eight numbers flat, as Pillow takes them - and size = (width, height) of the OUTPUT.  Computed by the C helper hipdec_quad_map with Pillow's own
    arithmetic, coefficient for coefficient."""
    lib = _bind(load_library())
    c = list(corners)
    c = [float(v) for v in c] if len(c) == 8 else [float(v) for p in c for v in p]
    if len(c) != 8:
        raise ValueError("quad_map takes four (x, y) corners: nw, sw, se, ne")
    out = TensorProjection()
    check(lib.hipdec_quad_map((C.c_double * 8)(*c), int(size[0]), int(size[1]), C.byref(out)))
    return out


def project_stats():
    """(launches of the projective kernel - one per projected call that wrote anything -, the entries they wrote) since load"""
    lib = _bind(load_library())
    a, b = C.c_uint64(), C.c_uint64()
    lib.hipdec_project_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def _to_tensor_projected(self, lib_call, size, maps, entries, src_size, warp_filter, fill, fill_domain, orientations, filter, dtype, layout, mean, std, scale,
                         bias, out, stream):
    n = self.n if entries is None else len(entries)
    wd = warp_desc(size if src_size is None else src_size, warp_filter)
    marr = tensor_projections(maps, n)
    f = None if fill is None else tensor_fill(fill, fill_domain)
    codes = None if orientations is None else _orientation_array(orientations, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: lib_call(h, desc, arr, codes, C.byref(wd), marr, f, n_, ptr, room, stream_)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)


# hipdec_photo_opcode: the photometric operations (PIL.ImageEnhance.* / PIL.ImageOps.* on the 8-bit picture, bit for bit)
PHOTO_BRIGHTNESS, PHOTO_COLOR, PHOTO_CONTRAST, PHOTO_SHARPNESS, PHOTO_POSTERIZE, PHOTO_SOLARIZE, PHOTO_INVERT, PHOTO_AUTOCONTRAST, PHOTO_EQUALIZE = range(1, 10)
PHOTO_MAX_OPS = 4
PHOTO_OPS = {"brightness": PHOTO_BRIGHTNESS, "color": PHOTO_COLOR, "contrast": PHOTO_CONTRAST, "sharpness": PHOTO_SHARPNESS, "posterize": PHOTO_POSTERIZE,
             "solarize": PHOTO_SOLARIZE, "invert": PHOTO_INVERT, "autocontrast": PHOTO_AUTOCONTRAST, "equalize": PHOTO_EQUALIZE}


def photo_chain(*ops):
    """hipdec_photo_chain from up to PHOTO_MAX_OPS operations, applied in order: ("contrast", 1.3), ("posterize", 4), "equalize", (PHOTO_INVERT,) - a name of
    PHOTO_OPS or a PHOTO_* constant, with its value where it takes one (the factor, the bits, the threshold)"""
    if len(ops) > PHOTO_MAX_OPS:
        raise ValueError("a chain has at most %d operations, not %d" % (PHOTO_MAX_OPS, len(ops)))
    ch = PhotoChain()
    ch.n_ops = len(ops)
    for k, o in enumerate(ops):
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        if not 1 <= len(o) <= 2:
            raise ValueError("an operation is a name or (name, value), not %r" % (o,))
        if isinstance(o[0], str) and o[0].lower() not in PHOTO_OPS:
            raise ValueError("unknown photometric operation %r" % (o[0],))
        ch.ops[k].op = PHOTO_OPS[o[0].lower()] if isinstance(o[0], str) else int(o[0])
        ch.ops[k].value = float(o[1]) if len(o) == 2 else 0.0
    return ch


def photo_chains(chains, n=None):
    """a ctypes array of hipdec_photo_chain from PhotoChain objects or sequences of operations (photo_chain's arguments)"""
    chains = list(chains)
    if n is not None and len(chains) != n:
        raise ValueError("%d chains for %d entries" % (len(chains), n))
    arr = (PhotoChain * max(len(chains), 1))()
    for k, ch in enumerate(chains):
        arr[k] = ch if isinstance(ch, PhotoChain) else photo_chain(*ch)
    return arr


def photo_desc(src_size):
    """hipdec_photo_desc for src_size = (width, height) of the samples"""
    return PhotoDesc(int(src_size[0]), int(src_size[1]), (C.c_int * 2)(0, 0))


def photo_stats():
    """(photo calls that wrote anything, the entries they wrote, launches of k_photo_hist and k_photo_apply together) since load"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_photo_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _to_tensor_photo(self, lib_call, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale, bias, out, stream):
    n = self.n if entries is None else len(entries)
    pd = photo_desc(size)
    carr = photo_chains(chains, n)
    codes = None if orientations is None else _orientation_array(orientations, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: lib_call(h, desc, arr, codes, C.byref(pd), carr, n_, ptr, room, stream_)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)


# the augment stage (hipdec_tensor_augment): the photo stage's operations, Pillow's hue shift and ImageFilter.GaussianBlur, chains of up to eight
AUGMENT_HUE, AUGMENT_GAUSSIAN_BLUR = 16, 17
AUGMENT_MAX_OPS = 8
AUGMENT_BLUR_MAX_RADIUS = 8.0
AUGMENT_OPS = dict(PHOTO_OPS, hue=AUGMENT_HUE, gaussian_blur=AUGMENT_GAUSSIAN_BLUR)


def augment_chain(*ops):
    """hipdec_augment_chain from up to AUGMENT_MAX_OPS operations, applied in order: photo_chain's operations, ("hue", d) with the integer shift d of
    0 .. 255 (hue_shift(hue_factor) for torchvision's factor) and ("gaussian_blur", radius) with Pillow's radius, 0 .. AUGMENT_BLUR_MAX_RADIUS"""
    if len(ops) > AUGMENT_MAX_OPS:
        raise ValueError("a chain has at most %d operations, not %d" % (AUGMENT_MAX_OPS, len(ops)))
    ch = AugmentChain()
    ch.n_ops = len(ops)
    for k, o in enumerate(ops):
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        if not 1 <= len(o) <= 2:
            raise ValueError("an operation is a name or (name, value), not %r" % (o,))
        if isinstance(o[0], str) and o[0].lower() not in AUGMENT_OPS:
            raise ValueError("unknown augment operation %r" % (o[0],))
        ch.ops[k].op = AUGMENT_OPS[o[0].lower()] if isinstance(o[0], str) else int(o[0])
        ch.ops[k].value = float(o[1]) if len(o) == 2 else 0.0
    return ch


def augment_chains(chains, n=None):
    """a ctypes array of hipdec_augment_chain from AugmentChain objects or sequences of operations (augment_chain's arguments)"""
    chains = list(chains)
    if n is not None and len(chains) != n:
        raise ValueError("%d chains for %d entries" % (len(chains), n))
    arr = (AugmentChain * max(len(chains), 1))()
    for k, ch in enumerate(chains):
        arr[k] = ch if isinstance(ch, AugmentChain) else augment_chain(*ch)
    return arr


def hue_shift(hue_factor):
    """the integer shift of ("hue", d) for the hue_factor of torchvision's adjust_hue on PIL images, -0.5 .. 0.5: int(hue_factor * 255), truncated
    toward zero, then mod 256 (the library's own statement of that convention; the operation itself is pinned to Pillow)"""
    if not -0.5 <= float(hue_factor) <= 0.5:
        raise ValueError("hue_factor %r is not in [-0.5, 0.5]" % (hue_factor,))
    return int(float(hue_factor) * 255) % 256


def gaussian_box(radius):
    """(r, ww, fw) of hipdec_gaussian_box: the extended box ImageFilter.GaussianBlur(radius) runs three times along each axis (host only)"""
    lib = _bind(load_library())
    r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
    check(lib.hipdec_gaussian_box(float(radius), C.byref(r), C.byref(ww), C.byref(fw)))
    return r.value, ww.value, fw.value


def augment_stats():
    """(augment calls that wrote anything, the entries they wrote, all kernel launches of the stage) since load"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_augment_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _to_tensor_augmented(self, lib_call, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale, bias, out, stream):
    n = self.n if entries is None else len(entries)
    pd = photo_desc(size)
    carr = augment_chains(chains, n)
    codes = None if orientations is None else _orientation_array(orientations, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: lib_call(h, desc, arr, codes, C.byref(pd), carr, n_, ptr, room, stream_)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)


# the recipe stage (hipdec_tensor_recipe): augment chains with affine steps - RandAugment / TrivialAugment / AutoAugment per sample in one call
RECIPE_AFFINE = 32
RECIPE_OPS = dict(AUGMENT_OPS, affine=RECIPE_AFFINE)


def shear_matrix(sx, sy=0.0):
    """(1, sx, 0, sy, 1, 0): PIL's AFFINE data of timm's and torchvision's PIL-path ShearX (sy = 0) and ShearY (sx = 0), exact - the literal tuple they hand
    to Image.transform.  (The library's own statement of that convention: neither timm nor torchvision is installed where this library is tested; the
    transform itself is pinned to Pillow.)"""
    return (1.0, float(sx), 0.0, float(sy), 1.0, 0.0)


def translate_matrix(tx, ty=0.0):
    """(1, 0, tx, 0, 1, ty): PIL's AFFINE data of timm's and torchvision's PIL-path TranslateX / TranslateY by tx / ty pixels, exact (the library's own
    statement of that convention, as shear_matrix)"""
    return (1.0, 0.0, float(tx), 0.0, 1.0, float(ty))


def recipe_affine(map, filter=SCALE_BILINEAR, fill=0):
    """hipdec_recipe_affine: PIL's AFFINE data (six numbers or a TensorMap), the warp filter of this operation (SCALE_NEAREST, SCALE_BILINEAR or
    SCALE_BICUBIC) and Pillow's fillcolor - one integer 0 .. 255 for all channels, or three"""
    fill = [int(fill)] * 3 if isinstance(fill, (int, np.integer)) else [int(v) for v in fill]
    if len(fill) != 3:
        raise ValueError("a fill is one integer or three, not %r" % (fill,))
    return RecipeAffine(tensor_maps([map])[0], int(filter), (C.c_int * 3)(*fill))


def recipe_chain(*ops, affines=None):
    """(chain, affines): a hipdec_augment_chain for the recipe stage from up to AUGMENT_MAX_OPS operations, applied in order - augment_chain's operations
    and ("affine", map, filter, fill) as recipe_affine takes them (filter and fill may be left out) -, and the list of RecipeAffine records its affine
    steps index.  Pass the list of an earlier chain as `affines` to collect the records of all chains of a call in one list."""
    if len(ops) > AUGMENT_MAX_OPS:
        raise ValueError("a chain has at most %d operations, not %d" % (AUGMENT_MAX_OPS, len(ops)))
    affines = [] if affines is None else affines
    ch = AugmentChain()
    ch.n_ops = len(ops)
    for k, o in enumerate(ops):
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        if isinstance(o[0], str) and o[0].lower() not in RECIPE_OPS:
            raise ValueError("unknown recipe operation %r" % (o[0],))
        op = RECIPE_OPS[o[0].lower()] if isinstance(o[0], str) else int(o[0])
        if op == RECIPE_AFFINE:
            if not 2 <= len(o) <= 4:
                raise ValueError("an affine operation is (\"affine\", map[, filter[, fill]]), not %r" % (o,))
            affines.append(o[1] if isinstance(o[1], RecipeAffine) and len(o) == 2 else recipe_affine(*o[1:]))
            ch.ops[k].op, ch.ops[k].value = op, float(len(affines) - 1)
            continue
        if not 1 <= len(o) <= 2:
            raise ValueError("an operation is a name or (name, value), not %r" % (o,))
        ch.ops[k].op = op
        ch.ops[k].value = float(o[1]) if len(o) == 2 else 0.0
    return ch, affines


def recipe_chains(chains, n=None):
    """(a ctypes array of hipdec_augment_chain, a ctypes array of hipdec_recipe_affine, n_affines) from sequences of operations (recipe_chain's
    arguments): what the recipe entry points take"""
    chains = list(chains)
    if n is not None and len(chains) != n:
        raise ValueError("%d chains for %d entries" % (len(chains), n))
    arr = (AugmentChain * max(len(chains), 1))()
    affines = []
    for k, ch in enumerate(chains):
        arr[k] = recipe_chain(*ch, affines=affines)[0]
    aarr = (RecipeAffine * max(len(affines), 1))(*affines)
    return arr, aarr, len(affines)


def recipe_stats():
    """(recipe calls that wrote anything, the entries they wrote, all kernel launches of the stage, the affine steps among the entries' steps) since load"""
    lib = _bind(load_library())
    v = [C.c_uint64() for _ in range(4)]
    lib.hipdec_recipe_stats(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def _to_tensor_recipe(self, lib_call, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale, bias, out, stream):
    n = self.n if entries is None else len(entries)
    pd = photo_desc(size)
    carr, aarr, n_aff = recipe_chains(chains, n)
    codes = None if orientations is None else _orientation_array(orientations, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: lib_call(h, desc, arr, codes, C.byref(pd), carr, aarr, n_aff, n_, ptr, room, stream_)
    return _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)


def fit_within(width, height, size):
    """The thumbnail size examples/heif_thumbnailer.cc:172-186 computes: the image as it is when both sides fit into `size`, else the longer
    side becomes `size` and the other one follows with integer division (which may give 0: the thumbnailer refuses that, and so does
    every scaled entry point here)."""
    if width <= size and height <= size:
        return width, height
    if width > height:
        return size, height * size // width
    return width * size // height, size


def _to_tensor(self, call, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations=None, placed=None, canvases=None):
    """Batch.to_tensor / Album.to_tensor: the description, the output buffer (DeviceBuffer or torch.Tensor) and the stream, then `call` (the oriented
    entry point when `orientations` is given; the placed one with placed = (places, fill, fill_domain, mask)); canvases: the samples of the tensor and
    of the mask where they are not one per entry (to_tensor_composed)"""
    n = self.n if entries is None else len(entries)
    n_out = n if canvases is None else canvases
    self._tensor_mask = None      # (the mask of THIS call, or none: tensor_mask_to_host() never hands back an earlier call's)
    last_mask = None
    if placed is not None:
        places, fill, fill_domain, mask = placed
        codes = None if orientations is None else _orientation_array(orientations, n)
        parr = None if places is None else tensor_places(places, n)
        f = None if fill is None else tensor_fill(fill, fill_domain)
        placed_call, mask_ptr = call, [None]
        call = lambda h, desc, arr, n, ptr, room, stream: placed_call(h, desc, arr, codes, parr, f, mask_ptr[0], n, ptr, room, stream)
    elif orientations is not None:
        codes = _orientation_array(orientations, n)
        oriented = call
        call = lambda h, desc, arr, n, ptr, room, stream: oriented(h, desc, arr, codes, n, ptr, room, stream)
    d0 = self.info(0)
    max_value = (1 << d0["bit_depth_luma"]) - 1 if (dtype != "uint8" and d0["bit_depth_luma"] > 8) else 255
    sc, bi = tensor_scale_bias(mean, std, scale, bias, max_value)
    desc = tensor_desc(size, dtype, layout, filter, sc, bi)
    shape = tensor_shape(n_out, size, layout)
    nbytes = int(np.prod(shape)) * np.dtype(_TENSOR_NUMPY[dtype]).itemsize
    arr = None if entries is None else tensor_entries(entries)
    host_wait = False
    if out is None:
        torch = _torch_gpu()
        out = torch.empty(shape, dtype=getattr(torch, dtype), device="cuda") if torch is not None else DeviceBuffer(max(nbytes, 1))
    if isinstance(out, DeviceBuffer):
        ptr, room = out.ptr, out.nbytes
    else:
        import torch
        if not isinstance(out, torch.Tensor) or not out.is_cuda:
            raise TypeError("out must be a DeviceBuffer or a CUDA / HIP torch.Tensor")
        if tuple(out.shape) != shape:
            raise ValueError("out has shape %s, the tensor has %s" % (tuple(out.shape), shape))
        if out.dtype != getattr(torch, dtype):
            raise ValueError("out has dtype %s, the tensor has %s" % (out.dtype, dtype))
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        ptr, room = out.data_ptr(), nbytes
        if stream is None:
            ts = torch.cuda.current_stream(out.device)
            stream = ts.cuda_stream or None
            if stream is None:
                # torch's legacy default stream has no handle the C ABI could name (NULL selects the library's own stream): order the two
                # on the host - what torch has queued for `out` first, and the tensor is complete when this call returns
                ts.synchronize()
                host_wait = True
    if placed is not None and mask is not None and mask is not False:
        mshape = (n_out, int(size[1]), int(size[0]))
        if mask is True:
            if isinstance(out, DeviceBuffer):
                mask = DeviceBuffer(max(int(np.prod(mshape)), 1))
            else:
                import torch
                mask = torch.empty(mshape, dtype=torch.uint8, device=out.device)
        if isinstance(mask, DeviceBuffer):
            if mask.nbytes < int(np.prod(mshape)):
                raise ValueError("mask has %d bytes, the mask tensor has %d" % (mask.nbytes, int(np.prod(mshape))))
            mask_ptr[0] = mask.ptr
        else:
            import torch
            if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.uint8:
                raise TypeError("mask must be True, a DeviceBuffer or a CUDA / HIP torch.Tensor of uint8")
            if tuple(mask.shape) != mshape or not mask.is_contiguous():
                raise ValueError("mask must be contiguous with shape %s" % (mshape,))
            mask_ptr[0] = mask.data_ptr()
        last_mask = (mask, mshape, stream)
    check(call(self._h, C.byref(desc), arr, n, ptr, room, stream))
    self._tensor_mask = last_mask
    if host_wait:
        check(self._lib.hipdec_stream_synchronize(None))
    self._tensor = (out, shape, _TENSOR_NUMPY[dtype], stream)
    return out


class DecodedImage:
    def __init__(self, info, planes):
        self.info = info
        self.planes = planes
        self.nclx = (info["colour_primaries"], info["transfer_characteristics"], info["matrix_coeffs"], info["full_range_flag"])


class HipDecoder:
    def __init__(self, strict_decoding=False, max_image_size_pixels=0):
        self._lib = _bind(load_library())
        self._h = C.c_void_p()
        check(self._lib.hipdec_decoder_new(C.byref(self._h), int(strict_decoding), int(max_image_size_pixels)))

    def push_data(self, data: bytes):
        check(self._lib.hipdec_decoder_push_data(self._h, data, len(data)))

    def flush_data(self):
        return None

    def decode_next_image(self):
        """Returns a DecodedImage, or None when there is nothing (more) to deliver."""
        info = ImageInfo()
        rc = self._lib.hipdec_decoder_decode(self._h, C.byref(info))
        if rc == -7:  # HIPDEC_ERR_NO_IMAGE
            return None
        check(rc)
        d = _info_dict(info)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        planes = []
        for c in range(3 if d["chroma_format_idc"] else 1):
            w, h = (d["width"], d["height"]) if c == 0 else (d["chroma_width"], d["chroma_height"])
            a = np.empty((h, w), dt)
            check(self._lib.hipdec_decoder_read_plane(self._h, c, a.ctypes.data, w * a.itemsize))
            planes.append(a)
        return DecodedImage(d, planes)

    def _read_planes(self, info):
        d = _info_dict(info)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        planes = []
        for c in range(3 if d["chroma_format_idc"] else 1):
            w, h = (d["width"], d["height"]) if c == 0 else (d["chroma_width"], d["chroma_height"])
            a = np.empty((h, w), dt)
            check(self._lib.hipdec_decoder_read_plane(self._h, c, a.ctypes.data, w * a.itemsize))
            planes.append(a)
        return DecodedImage(d, planes)

    def next_picture(self, flush=False, user_data=None):
        """decode_next_image2 with output order (hipdec_decoder_next_picture): decodes the pushed sample if one is pending and returns
        (DecodedImage, user_data) of the next picture in OUTPUT order, or None while the bumping process holds it back (B pictures)."""
        if user_data is not None:
            self._lib.hipdec_decoder_set_user_data.argtypes = [C.c_void_p, C.c_size_t]
            self._lib.hipdec_decoder_set_user_data.restype = None
            self._lib.hipdec_decoder_set_user_data(self._h, int(user_data))
        self._lib.hipdec_decoder_next_picture.argtypes = [C.c_void_p, C.c_int, C.POINTER(ImageInfo), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        info, have, ud = ImageInfo(), C.c_int(0), C.c_size_t(0)
        check(self._lib.hipdec_decoder_next_picture(self._h, 1 if flush else 0, C.byref(info), C.byref(have), C.byref(ud)))
        if not have.value:
            return None
        return self._read_planes(info), ud.value

    def free(self):
        if self._h:
            self._lib.hipdec_decoder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Batch:
    """Many independent coded items (grid tiles, batches of stills) decoded by one set of launches."""

    def __init__(self, streams, max_image_size_pixels=0, recycle=None):
        """recycle: a batch of the same shape whose planes have been consumed; its arena is taken over (a stream of batches)"""
        self._lib = _bind(load_library())
        self._keep = [bytes(s) for s in streams]
        n = len(self._keep)
        arr = (C.c_char_p * n)(*self._keep)
        sizes = (C.c_size_t * n)(*[len(s) for s in self._keep])
        self._h = C.c_void_p()
        if recycle is None:
            check(self._lib.hipdec_batch_create(C.byref(self._h), n, arr, sizes, int(max_image_size_pixels)))
        else:
            check(self._lib.hipdec_batch_create_recycling(C.byref(self._h), n, arr, sizes, int(max_image_size_pixels), recycle._h))
        self.n = n

    def info(self, i):
        info = ImageInfo()
        check(self._lib.hipdec_batch_info(self._h, i, C.byref(info)))
        return _info_dict(info)

    def run(self, stream=None):
        check(self._lib.hipdec_batch_run(self._h, stream))

    def status(self):
        check(self._lib.hipdec_batch_status(self._h))

    def planes(self, i):
        d = self.info(i)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        out = []
        for c in range(3 if d["chroma_format_idc"] else 1):
            w, h = (d["width"], d["height"]) if c == 0 else (d["chroma_width"], d["chroma_height"])
            a = np.empty((h, w), dt)
            check(self._lib.hipdec_batch_read_plane(self._h, i, c, a.ctypes.data, w * a.itemsize))
            out.append(a)
        return out

    def tap(self, i, c):
        """deblocked (pre-SAO) picture at coded size — debug tap"""
        d = self.info(i)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        cf = d["chroma_format_idc"]
        subw, subh = (1, 1) if c == 0 else ((1 if cf == 3 else 2), (2 if cf == 1 else 1))
        w, h = d["coded_width"] // subw, d["coded_height"] // subh
        a = np.empty((h, w), dt)
        check(self._lib.hipdec_batch_read_tap(self._h, i, 1, c, a.ctypes.data, w * a.itemsize))
        return a

    def maps(self, i):
        d = self.info(i)
        uw, uh = (d["coded_width"] + 3) // 4, (d["coded_height"] + 3) // 4
        names = ["log2_tb", "log2_cb", "intra_luma", "intra_chroma", "qp_y", "flags"]
        arrs = [np.zeros((uh, uw), np.int8 if n == "qp_y" else np.uint8) for n in names]
        check(self._lib.hipdec_batch_read_maps(self._h, i, *[a.ctypes.data for a in arrs], uw * uh))
        return dict(zip(names, arrs))

    def to_rgb(self, i, out_chroma=10):
        """fused colour stage on the device planes of item i; returns the interleaved rows (uint8)."""
        d = self.info(i)
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        w, h = d["width"], d["height"]
        buf = DeviceBuffer(w * h * bpp)
        check(self._lib.hipdec_batch_to_rgb(self._h, i, out_chroma, buf.ptr, w * bpp, None))
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((h, w * bpp), np.uint8)

    def alloc_rgb(self, out_chroma=10):
        """pre-allocates one interleaved output buffer per item for to_rgb_all()"""
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        self._rgb = []
        for i in range(self.n):
            d = self.info(i)
            self._rgb.append((DeviceBuffer(d["width"] * d["height"] * bpp), d["width"] * bpp, d["height"]))
        self._rgb_chroma = out_chroma
        self._rgb_ptrs = (C.c_void_p * self.n)(*[buf.ptr for buf, _, _ in self._rgb])
        self._rgb_strides = (C.c_size_t * self.n)(*[stride for _, stride, _ in self._rgb])

    def rgb_state(self):
        """the pre-allocated output buffers (device memory owned by Python objects), to hand to another batch of the same shape"""
        return (self._rgb, self._rgb_chroma, self._rgb_ptrs, self._rgb_strides)

    def use_rgb(self, state):
        self._rgb, self._rgb_chroma, self._rgb_ptrs, self._rgb_strides = state

    def to_rgb_all(self, stream=None):
        """asynchronous: fused colour stage over every item's planes into the pre-allocated buffers, ONE launch"""
        check(self._lib.hipdec_batch_to_rgb_all(self._h, self._rgb_chroma, self._rgb_ptrs, self._rgb_strides, stream))

    def run_rgb(self, stream=None):
        """asynchronous: decode + colour stage into the pre-allocated buffers as ONE call (for 8-bit 4:2:0 -> RGB24 the colour conversion is
        fused into the SAO kernel's store path)"""
        check(self._lib.hipdec_batch_run_rgb(self._h, self._rgb_chroma, self._rgb_ptrs, self._rgb_strides, stream))

    def to_rgb_scaled(self, i, width, height, filter=SCALE_BOX, out_chroma=10):
        """item i as interleaved rows of width x height pixels straight from its decoded planes (one fused scale + colour kernel).  filter: SCALE_NEAREST,
        SCALE_BOX, or - out_chroma 10 only - SCALE_BILINEAR / SCALE_BICUBIC (PIL.Image.resize of to_rgb(i, 10), bit for bit)"""
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        buf = DeviceBuffer(max(1, width) * max(1, height) * bpp)
        check(self._lib.hipdec_batch_to_rgb_scaled(self._h, i, out_chroma, width, height, filter, buf.ptr, width * bpp, None))
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((height, width * bpp), np.uint8)

    def alloc_rgb_scaled(self, sizes, out_chroma=10):
        """pre-allocates one scaled output buffer per item for to_rgb_scaled_all(); sizes: (width, height) per item, or one pair for all"""
        if len(sizes) == 2 and not hasattr(sizes[0], "__len__"):
            sizes = [tuple(sizes)] * self.n
        assert len(sizes) == self.n
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        self._srgb = [(DeviceBuffer(w * h * bpp), w * bpp, h) for w, h in sizes]
        self._srgb_chroma = out_chroma
        self._srgb_w = (C.c_int * self.n)(*[w for w, _ in sizes])
        self._srgb_h = (C.c_int * self.n)(*[h for _, h in sizes])
        self._srgb_ptrs = (C.c_void_p * self.n)(*[buf.ptr for buf, _, _ in self._srgb])
        self._srgb_strides = (C.c_size_t * self.n)(*[stride for _, stride, _ in self._srgb])

    def to_rgb_scaled_all(self, filter=SCALE_BOX, stream=None, orientations=None):
        """asynchronous: every item scaled to its pre-allocated size, ONE launch.  orientations: one hipdec_orientation code per item - the sizes given to
        alloc_rgb_scaled() are then sizes of the DISPLAYED pictures (RGB24 only).  filter: SCALE_NEAREST, SCALE_BOX, or - RGB24 only - SCALE_BILINEAR /
        SCALE_BICUBIC (PIL.Image.resize bit for bit)"""
        if orientations is not None:
            check(self._lib.hipdec_batch_to_rgb_scaled_oriented_all(self._h, self._srgb_chroma, _orientation_array(orientations, self.n), self._srgb_w, self._srgb_h,
                                                                    filter, self._srgb_ptrs, self._srgb_strides, stream))
            return
        check(self._lib.hipdec_batch_to_rgb_scaled_all(self._h, self._srgb_chroma, self._srgb_w, self._srgb_h, filter, self._srgb_ptrs,
                                                       self._srgb_strides, stream))

    def to_tensor(self, size, entries=None, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, filter=SCALE_BOX, out=None,
                  stream=None, orientations=None, places=None, fill=None, fill_domain="component", mask=None, frames=None):
        """asynchronous: crop windows of the decoded pictures, scaled to size = (width, height), optionally flipped, as ONE dense tensor of shape
        (N, 3, height, width) ("NCHW") or (N, height, width, 3) ("NHWC") written by one fused kernel (hipdec_batch_to_tensor).

        entries: (item, left, top, width, height[, flip]) tuples - the window in luma samples, all zeros after `item` for the whole picture, several
        entries may name one item (center_crop_entry, random_resized_crop_entries) - or None: every item whole, in order.
        dtype: "float16" | "bfloat16" | "float32" | "uint8".  Element = float32(V) * scale[c] + bias[c] (uint8: V itself), V the 8-bit component value,
        or for float dtypes from sources above 8 bits the native-depth one.  scale / bias: a number or three per channel; or mean / std in the usual
        0..1 convention, folded in float32 exactly as tensor_scale_bias() states:
            scale[c] = float32(1) / (float32(max_value) * float32(std[c])),  bias[c] = -float32(mean[c]) / float32(std[c]),
        max_value = 255, or 2^bits - 1 of item 0 for float dtypes from sources above 8 bits.
        out: a DeviceBuffer of at least the tensor's bytes (returned as it is; tensor_to_host() reads it back as a NumPy array), or a contiguous
        CUDA / HIP torch.Tensor of the tensor's shape and dtype (its data_ptr() is written; the stream defaults to torch's current stream - when that
        is torch's legacy default stream the call waits on the host instead), or None: a torch tensor where torch sees a GPU, a DeviceBuffer elsewhere.
        orientations: one hipdec_orientation code per entry (hipdec_batch_to_tensor_oriented): `size` is then the size of the DISPLAYED sample, windows
        stay in the stored picture (stored_window() maps a displayed window), and an entry's flip mirrors the displayed sample.
        filter: SCALE_NEAREST, SCALE_BOX, or SCALE_BILINEAR / SCALE_BICUBIC: V = PIL.Image.resize of the window of the 8-bit RGB picture (to_rgb(i, 10)),
        bit for bit - what torchvision's Resize / RandomResizedCrop compute on PIL images; from sources above 8 bits with dtype "uint8" only.
        places / fill / mask (hipdec_batch_to_tensor_placed; any of them selects it): `size` is then the size of the CANVAS of every entry, places one
        (x, y, width, height) rectangle per entry - the displayed sample is written there at that size (letterbox_places()), None: the whole canvas -
        and the rest of the canvas holds `fill`: a number or three per channel, with fill_domain "component" a pixel's component value (normalised as
        pixels are: fill=114 is the usual grey) or "element" the tensor element itself (0.0: zero after normalisation); default component 0.
        mask: a DeviceBuffer or a uint8 torch.Tensor of shape (N, height, width), or True to allocate one - 1 where the canvas is padding, 0 inside the
        rectangle (tensor_mask_to_host() reads the mask of the LAST call back; it raises when that call wrote none).  The mask is written on the stream the
        tensor is written on: `stream`, or - stream None - torch's current stream when `out` is a torch.Tensor and the library's own stream when `out`
        is a DeviceBuffer, whatever the mask is; a torch mask next to a DeviceBuffer `out` therefore needs `stream=` (or synchronize()) to be ordered
        with torch's work.
        frames (hipdec_batch_to_tensor_framed; instead of places): one (x, y, width, height) rectangle per entry that may leave the canvas on any side -
        x and y may be negative - of which the part on the canvas is computed and written: resize-then-crop (resize_crop_places()), RandomCrop with
        padding (random_crop_places()).  fill / fill_domain / mask as with places, the mask 0 on the visible part."""
        if frames is not None:
            if places is not None:
                raise ValueError("places and frames are mutually exclusive")
            return _to_tensor(self, self._lib.hipdec_batch_to_tensor_framed, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations,
                              (frames, fill, fill_domain, mask))
        if places is not None or fill is not None or mask is not None:
            return _to_tensor(self, self._lib.hipdec_batch_to_tensor_placed, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations,
                              (places, fill, fill_domain, mask))
        if orientations is not None:
            return _to_tensor(self, self._lib.hipdec_batch_to_tensor_oriented, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations)
        return _to_tensor(self, self._lib.hipdec_batch_to_tensor, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)

    def to_tensor_composed(self, size, tiles, entries=None, n_canvases=None, orientations=None, fill=None, fill_domain="component", mask=None, filter=SCALE_BOX,
                           dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """asynchronous: SEVERAL entries per canvas - mosaic, CutMix, contact sheets - as ONE tensor of n_canvases canvases of size = (width, height)
        (hipdec_batch_to_tensor_composed).  tiles: one (canvas, place, clip) per entry - the canvas it belongs to, the rectangle of its resized,
        displayed sample in canvas coordinates (it may leave the canvas) and the rectangle of the canvas it may write (None or all zeros: the whole canvas);
        mosaic_tiles(), sheet_tiles() and cutmix_tiles() make them.  Later entries lie on top; pixels nobody owns hold `fill` (fill / fill_domain as in
        to_tensor(places=)), and mask - a DeviceBuffer, a uint8 torch.Tensor of shape (n_canvases, height, width) or True - is 1 there.  n_canvases None:
        the largest canvas index + 1.  Inside what an entry owns the canvas holds what to_tensor(place size, ..., orientations=) writes for it.  `out`,
        `stream`, tensor_to_host() and tensor_mask_to_host() as in to_tensor.  One launch of the picture kernels and at most one of the cover kernel."""
        return _to_tensor_composed(self, self._lib.hipdec_batch_to_tensor_composed, size, tiles, entries, n_canvases, orientations, fill, fill_domain, mask, filter,
                                   dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_warped(self, size, maps, entries=None, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", orientations=None,
                         filter=SCALE_BILINEAR, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """asynchronous: to_tensor with one affine warp per entry, Pillow-exact (hipdec_batch_to_tensor_warped).  Entry e is first resized as
        to_tensor(src_size, entries, dtype="uint8", layout="NHWC", filter=filter, orientations=orientations) resizes it - src_size defaults to `size` -
        and that 8-bit picture then goes through PIL.Image.transform(size, AFFINE, maps[e], warp_filter, fillcolor=fill) bit for bit, normalised as
        to_tensor normalises.  maps: six numbers per entry (rotate_matrix(), affine_matrix(), or any AFFINE data); warp_filter: SCALE_NEAREST,
        SCALE_BILINEAR or SCALE_BICUBIC; fill / fill_domain as in to_tensor(places=).  Sources above 8 bits: dtype "uint8" only.  `out`, `stream` and
        tensor_to_host() as in to_tensor.  One resize launch and one warp launch per call."""
        return _to_tensor_warped(self, self._lib.hipdec_batch_to_tensor_warped, size, maps, entries, src_size, warp_filter, fill, fill_domain, orientations,
                                 filter, dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_projected(self, size, maps, entries=None, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", orientations=None,
                            filter=SCALE_BILINEAR, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """asynchronous: to_tensor with one PERSPECTIVE or QUAD transform per entry, Pillow-exact (hipdec_batch_to_tensor_projected).  Entry e is first
        resized as to_tensor(src_size, entries, dtype="uint8", layout="NHWC", filter=filter, orientations=orientations) resizes it - src_size defaults to
        `size` - and that 8-bit picture then goes through PIL.Image.transform(size, PERSPECTIVE | QUAD, maps[e], warp_filter, fillcolor=fill) bit for bit,
        normalised as to_tensor normalises.  maps: per entry eight numbers (PERSPECTIVE data), a (kind, eight numbers) pair, or what perspective_map() /
        quad_map() return; the entries of a call may mix the kinds.  Everything else as in to_tensor_warped.  One resize launch and one projective launch
        per call."""
        return _to_tensor_projected(self, self._lib.hipdec_batch_to_tensor_projected, size, maps, entries, src_size, warp_filter, fill, fill_domain,
                                    orientations, filter, dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_photo(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                        scale=None, bias=None, out=None, stream=None):
        """asynchronous: to_tensor with one chain of photometric operations per entry, Pillow-exact (hipdec_batch_to_tensor_photo).  Entry e is first
        resized as to_tensor(size, entries, dtype="uint8", layout="NHWC", filter=filter, orientations=orientations) resizes it, and that 8-bit picture then
        goes through chains[e] - a PhotoChain or a sequence of operations as photo_chain takes them: ImageEnhance.Brightness / Color / Contrast /
        Sharpness, ImageOps.posterize / solarize / invert / autocontrast / equalize, bit for bit, each on the 8-bit result of the one before - and is
        normalised as to_tensor normalises.  The statistics contrast, autocontrast and equalize need are taken on the device.  Sources above 8 bits:
        dtype "uint8" only.  `out`, `stream` and tensor_to_host() as in to_tensor.  One resize launch, then at most two launches per chain step."""
        return _to_tensor_photo(self, self._lib.hipdec_batch_to_tensor_photo, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale,
                                bias, out, stream)

    def to_tensor_augmented(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                            scale=None, bias=None, out=None, stream=None):
        """asynchronous: to_tensor_photo with the augment stage's chains (hipdec_batch_to_tensor_augmented): up to AUGMENT_MAX_OPS operations per entry,
        the photometric ones plus ("hue", d) - Pillow's HSV round trip with a wrap-around shift of H, hue_shift(hue_factor) gives d - and
        ("gaussian_blur", radius) - PIL.ImageFilter.GaussianBlur(radius), radius 0 .. AUGMENT_BLUR_MAX_RADIUS -, bit for bit.  chains[e]: an AugmentChain or
        a sequence of operations as augment_chain takes them.  One resize launch, then at most four launches per chain step."""
        return _to_tensor_augmented(self, self._lib.hipdec_batch_to_tensor_augmented, size, chains, entries, orientations, filter, dtype, layout, mean, std,
                                    scale, bias, out, stream)

    def to_tensor_recipe(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                         scale=None, bias=None, out=None, stream=None):
        """asynchronous: to_tensor_augmented with affine steps inside the chains (hipdec_batch_to_tensor_recipe) - what RandAugment, TrivialAugment and
        AutoAugment draw per sample: chains[e] is a sequence of operations as recipe_chain takes them, augment_chain's plus ("affine", map, filter, fill) -
        PIL.Image.transform(size, AFFINE, map, filter, fillcolor=fill) of the 8-bit result of the step before, bit for bit, with the warp filter and the fill
        per operation (rotate_matrix, shear_matrix, translate_matrix give the maps).  One resize launch, then at most seven launches per chain step."""
        return _to_tensor_recipe(self, self._lib.hipdec_batch_to_tensor_recipe, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale,
                                 bias, out, stream)

    def to_tensor_packed(self, sizes, entries=None, patch=0, merge=1, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None,
                         filter=SCALE_BOX, orientations=None, offsets=None, out=None, stream=None):
        """asynchronous: every entry at its OWN displayed size sizes[e] = (width, height), all entries in one launch into one 1-D output
        (hipdec_batch_to_tensor_packed) - what native-resolution vision encoders take.  Sample e is what to_tensor(sizes[e], ..., orientations=) writes for
        the entry, stored from element offsets[e] on: densely in `layout` (patch 0), or as the sequence of its patch tokens (patch P >= 1, sizes multiples
        of P * merge): token t = ((gy // m) * (gw // m) + gx // m) * m * m + (gy % m) * m + gx % m of patch (gy, gx), inside a token Conv2d weight order
        (c, py, px) for "NCHW" and big_vision / NaFlex order (py, px, c) for "NHWC".  merge 2 is the token order of Qwen2-VL's image processor.
        offsets None: the samples back to back in entry order (packed_layout()).  Choosing the sizes stays with the caller.
        out: a DeviceBuffer, or a 1-D torch.Tensor (written on torch's current stream unless `stream` is given); None allocates one.
        Returns (out, offsets, grids) with grids[e] = (height / P, width / P) for patches, None for dense samples; out[offsets[0]:].view(-1, 3 * P * P)
        of back-to-back samples is the packed sequence.  tensor_packed_to_host() reads the result back."""
        return _to_tensor_packed(self, self._lib.hipdec_batch_to_tensor_packed, sizes, entries, patch, merge, dtype, layout, mean, std, scale, bias, filter,
                                 orientations, offsets, out, stream)

    tensor_packed_to_host = _tensor_packed_to_host

    def tensor_to_host(self):
        """the last to_tensor() result as a NumPy array of the tensor's shape (bfloat16 as uint16 bit patterns); waits for its stream"""
        out, shape, dt, stream = self._tensor
        check(self._lib.hipdec_stream_synchronize(stream))
        if isinstance(out, DeviceBuffer):
            return out.to_numpy(shape, dt)
        import torch
        t = out.view(torch.int16) if dt == np.uint16 else out
        a = t.cpu().numpy()
        return a.view(np.uint16) if dt == np.uint16 else a

    def tensor_mask_to_host(self):
        """the mask of the last placed to_tensor() as a NumPy uint8 array of shape (N, height, width); waits for its stream"""
        if getattr(self, "_tensor_mask", None) is None:
            raise RuntimeError("tensor_mask_to_host: the last to_tensor() wrote no mask (mask= was not given, or there has been no call)")
        mask, shape, stream = self._tensor_mask
        check(self._lib.hipdec_stream_synchronize(stream))
        if isinstance(mask, DeviceBuffer):
            return mask.to_numpy(shape, np.uint8)
        return mask.cpu().numpy()

    def tensor_block(self, entry, plane):
        """debug inspection (hipdec_batch_tensor_block): (device pointer, stride, x, y, width, height) of a plane of an entry of the last to_tensor()"""
        p, st = C.c_void_p(), C.c_size_t()
        x, y, w, h = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self._lib.hipdec_batch_tensor_block(self._h, entry, plane, C.byref(p), C.byref(st), C.byref(x), C.byref(y), C.byref(w), C.byref(h)))
        return p.value, st.value, x.value, y.value, w.value, h.value

    def rgb_scaled(self, i):
        buf, stride, h = self._srgb[i]
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((h, stride), np.uint8)

    def planes_scaled(self, i, width, height, filter=SCALE_BOX):
        """the planes of item i scaled as hipdec_image_scale does it (chroma planes at the subsampled size of the width x height image)"""
        d = self.info(i)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        cf = d["chroma_format_idc"]
        out = []
        for c in range(3 if cf else 1):
            w = width if c == 0 or cf == 3 else (width + 1) // 2
            h = height if c == 0 or cf != 1 else (height + 1) // 2
            a = np.empty((max(h, 0), max(w, 0)), dt)
            check(self._lib.hipdec_batch_read_plane_scaled(self._h, i, c, width, height, filter, a.ctypes.data, w * a.itemsize))
            out.append(a)
        return out

    def rgb(self, i):
        buf, stride, h = self._rgb[i]
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((h, stride), np.uint8)

    def timing_us(self):
        t = (C.c_float * 5)()
        check(self._lib.hipdec_batch_last_timing_us(self._h, t))
        return dict(parse=t[0], recon=t[1], deblock=t[2], sao=t[3], total=t[4])

    def timing_slots(self, n):
        check(self._lib.hipdec_batch_timing_slots(self._h, n))

    def slot_timing_us(self, slot):
        t = (C.c_float * 5)()
        check(self._lib.hipdec_batch_slot_timing_us(self._h, slot, t))
        return dict(parse=t[0], recon=t[1], deblock=t[2], sao=t[3], total=t[4])

    _KERNELS = ("parse", "residual", "recon", "deblock", "sao", "colour", "decode_total")

    def slot_kernel_timing_us(self, slot):
        """device time per kernel of the run recorded in `slot` (HIP events on the launch stream), microseconds"""
        t = (C.c_float * 8)()
        check(self._lib.hipdec_batch_slot_kernel_timing_us(self._h, slot, t))
        return {k: t[i] for i, k in enumerate(self._KERNELS)}

    def kernel_timing_us(self):
        """of the last run when the batch keeps one timing slot (the default)"""
        return self.slot_kernel_timing_us(0)

    def free(self):
        if self._h:
            self._lib.hipdec_batch_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def album_stats():
    """(albums created, their photos, paste launches - one per Album.run) since the library was loaded"""
    lib = _bind(load_library())
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.hipdec_album_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


class Album:
    """Many grid photos composed by one set of launches (hipdec_album_*): the tiles of all photos decode as ONE batch and ONE paste kernel puts every
    tile plane into its photo's canvas; the canvases feed the colour, scaled and tensor stages of Batch, one launch each."""

    def __init__(self, photos, max_image_size_pixels=0):
        """photos: (tile_streams, rows, cols, out_w, out_h) per photo, the tiles in grid ('dimg') order"""
        self._lib = _bind(load_library())
        self._keep = []
        desc = (AlbumPhoto * max(len(photos), 1))()
        for p, (tiles, rows, cols, out_w, out_h) in enumerate(photos):
            desc[p] = AlbumPhoto(int(rows), int(cols), int(out_w), int(out_h), len(self._keep), 0)
            self._keep += [bytes(t) for t in tiles]
        n = len(self._keep)
        arr = (C.c_char_p * max(n, 1))(*self._keep)
        sizes = (C.c_size_t * max(n, 1))(*[len(t) for t in self._keep])
        self._h = C.c_void_p()
        check(self._lib.hipdec_album_create(C.byref(self._h), len(photos), desc, arr, sizes, n, int(max_image_size_pixels)))
        self.n = len(photos)

    def info(self, p):
        info = ImageInfo()
        check(self._lib.hipdec_album_info(self._h, p, C.byref(info)))
        return _info_dict(info)

    def run(self, stream=None):
        """asynchronous: the launch set of all tiles + ONE paste launch"""
        check(self._lib.hipdec_album_run(self._h, stream))

    def status(self):
        check(self._lib.hipdec_album_status(self._h))

    def planes(self, p):
        """the composed planes of photo p (host arrays of the output size)"""
        d = self.info(p)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        out = []
        for c in range(3 if d["chroma_format_idc"] else 1):
            w, h = (d["width"], d["height"]) if c == 0 else (d["chroma_width"], d["chroma_height"])
            a = np.empty((h, w), dt)
            check(self._lib.hipdec_album_read_plane(self._h, p, c, a.ctypes.data, w * a.itemsize))
            out.append(a)
        return out

    def canvas_plane(self, p, c):
        """(device pointer, stride) of plane c of photo p's canvas"""
        ptr, st = C.c_void_p(), C.c_size_t()
        check(self._lib.hipdec_album_canvas_plane(self._h, p, c, C.byref(ptr), C.byref(st)))
        return ptr.value, st.value

    def alloc_rgb(self, out_chroma=10):
        """pre-allocates one interleaved output buffer per photo for to_rgb_all()"""
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        self._rgb = []
        for p in range(self.n):
            d = self.info(p)
            self._rgb.append((DeviceBuffer(d["width"] * d["height"] * bpp), d["width"] * bpp, d["height"]))
        self._rgb_chroma = out_chroma
        self._rgb_ptrs = (C.c_void_p * self.n)(*[buf.ptr for buf, _, _ in self._rgb])
        self._rgb_strides = (C.c_size_t * self.n)(*[stride for _, stride, _ in self._rgb])

    def to_rgb_all(self, stream=None):
        """asynchronous: fused colour stage over every photo's canvas into the pre-allocated buffers, ONE launch"""
        check(self._lib.hipdec_album_to_rgb_all(self._h, self._rgb_chroma, self._rgb_ptrs, self._rgb_strides, stream))

    def rgb(self, p):
        buf, stride, h = self._rgb[p]
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((h, stride), np.uint8)

    def alloc_rgb_scaled(self, sizes, out_chroma=10):
        """pre-allocates one scaled output buffer per photo for to_rgb_scaled_all(); sizes: (width, height) per photo, or one pair for all"""
        if len(sizes) == 2 and not hasattr(sizes[0], "__len__"):
            sizes = [tuple(sizes)] * self.n
        assert len(sizes) == self.n
        bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
        self._srgb = [(DeviceBuffer(w * h * bpp), w * bpp, h) for w, h in sizes]
        self._srgb_chroma = out_chroma
        self._srgb_w = (C.c_int * self.n)(*[w for w, _ in sizes])
        self._srgb_h = (C.c_int * self.n)(*[h for _, h in sizes])
        self._srgb_ptrs = (C.c_void_p * self.n)(*[buf.ptr for buf, _, _ in self._srgb])
        self._srgb_strides = (C.c_size_t * self.n)(*[stride for _, stride, _ in self._srgb])

    def to_rgb_scaled_all(self, filter=SCALE_BOX, stream=None, orientations=None):
        """asynchronous: every photo scaled to its pre-allocated size, ONE launch; orientations: as Batch.to_rgb_scaled_all"""
        if orientations is not None:
            check(self._lib.hipdec_album_to_rgb_scaled_oriented_all(self._h, self._srgb_chroma, _orientation_array(orientations, self.n), self._srgb_w, self._srgb_h,
                                                                    filter, self._srgb_ptrs, self._srgb_strides, stream))
            return
        check(self._lib.hipdec_album_to_rgb_scaled_all(self._h, self._srgb_chroma, self._srgb_w, self._srgb_h, filter, self._srgb_ptrs,
                                                       self._srgb_strides, stream))

    def rgb_scaled(self, p):
        buf, stride, h = self._srgb[p]
        check(self._lib.hipdec_stream_synchronize(None))
        return buf.to_numpy((h, stride), np.uint8)

    def to_tensor(self, size, entries=None, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, filter=SCALE_BOX, out=None,
                  stream=None, orientations=None, places=None, fill=None, fill_domain="component", mask=None, frames=None):
        """Batch.to_tensor over the composed photos: an entry's item names a photo, its window lies in the photo's output size"""
        if frames is not None:
            if places is not None:
                raise ValueError("places and frames are mutually exclusive")
            return _to_tensor(self, self._lib.hipdec_album_to_tensor_framed, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations,
                              (frames, fill, fill_domain, mask))
        if places is not None or fill is not None or mask is not None:
            return _to_tensor(self, self._lib.hipdec_album_to_tensor_placed, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations,
                              (places, fill, fill_domain, mask))
        if orientations is not None:
            return _to_tensor(self, self._lib.hipdec_album_to_tensor_oriented, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream, orientations)
        return _to_tensor(self, self._lib.hipdec_album_to_tensor, size, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)

    tensor_to_host = Batch.tensor_to_host
    tensor_mask_to_host = Batch.tensor_mask_to_host

    def to_tensor_composed(self, size, tiles, entries=None, n_canvases=None, orientations=None, fill=None, fill_domain="component", mask=None, filter=SCALE_BOX,
                           dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_composed over the composed photos (hipdec_album_to_tensor_composed)"""
        return _to_tensor_composed(self, self._lib.hipdec_album_to_tensor_composed, size, tiles, entries, n_canvases, orientations, fill, fill_domain, mask, filter,
                                   dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_warped(self, size, maps, entries=None, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", orientations=None,
                         filter=SCALE_BILINEAR, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_warped over the composed photos"""
        return _to_tensor_warped(self, self._lib.hipdec_album_to_tensor_warped, size, maps, entries, src_size, warp_filter, fill, fill_domain, orientations,
                                 filter, dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_projected(self, size, maps, entries=None, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", orientations=None,
                            filter=SCALE_BILINEAR, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_projected over the composed photos"""
        return _to_tensor_projected(self, self._lib.hipdec_album_to_tensor_projected, size, maps, entries, src_size, warp_filter, fill, fill_domain,
                                    orientations, filter, dtype, layout, mean, std, scale, bias, out, stream)

    def to_tensor_photo(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                        scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_photo over the composed photos"""
        return _to_tensor_photo(self, self._lib.hipdec_album_to_tensor_photo, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale,
                                bias, out, stream)

    def to_tensor_augmented(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                            scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_augmented over the composed photos"""
        return _to_tensor_augmented(self, self._lib.hipdec_album_to_tensor_augmented, size, chains, entries, orientations, filter, dtype, layout, mean, std,
                                    scale, bias, out, stream)

    def to_tensor_recipe(self, size, chains, entries=None, filter=SCALE_BILINEAR, orientations=None, dtype="float16", layout="NCHW", mean=None, std=None,
                         scale=None, bias=None, out=None, stream=None):
        """Batch.to_tensor_recipe over the composed photos"""
        return _to_tensor_recipe(self, self._lib.hipdec_album_to_tensor_recipe, size, chains, entries, orientations, filter, dtype, layout, mean, std, scale,
                                 bias, out, stream)

    def to_tensor_packed(self, sizes, entries=None, patch=0, merge=1, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None,
                         filter=SCALE_BOX, orientations=None, offsets=None, out=None, stream=None):
        """Batch.to_tensor_packed over the composed photos"""
        return _to_tensor_packed(self, self._lib.hipdec_album_to_tensor_packed, sizes, entries, patch, merge, dtype, layout, mean, std, scale, bias, filter,
                                 orientations, offsets, out, stream)

    tensor_packed_to_host = _tensor_packed_to_host

    def paste_timing_us(self):
        """device time of the paste launch of the last run(), microseconds"""
        t = C.c_float()
        check(self._lib.hipdec_album_paste_timing_us(self._h, C.byref(t)))
        return t.value

    def free(self):
        if self._h:
            self._lib.hipdec_album_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- clips (video loaders): include/heif_hipdec.h hipdec_clips_* ------------------------------------------------------------------------------------------
class _WarpStage:
    """what _to_tensor needs of a handle, for decoder.tensor_warp: n samples of 8 bits, no handle"""

    def __init__(self, lib, n):
        self._lib, self._h, self.n = lib, None, n

    def info(self, i):
        return {"bit_depth_luma": 8}

    tensor_to_host = Batch.tensor_to_host


def _tensor_map_stage(lib_call, make_maps, src, size, maps, src_size, warp_filter, fill, fill_domain, dtype, layout, mean, std, scale, bias, out, stream, to_host):
    """tensor_warp and tensor_project: the source, the maps, then the stage's call"""
    lib = _bind(load_library())
    maps = list(maps)
    n = len(maps)
    if isinstance(src, DeviceBuffer):
        if src_size is None:
            raise ValueError("a DeviceBuffer source needs src_size = (width, height)")
        sptr, sbytes = src.ptr, src.nbytes
    else:
        import torch
        if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8:
            raise TypeError("src must be a DeviceBuffer or a CUDA / HIP torch.Tensor of uint8")
        if src.dim() != 4 or src.shape[0] != n or src.shape[3] != 3 or not src.is_contiguous():
            raise ValueError("src must be contiguous with shape (%d, src_height, src_width, 3)" % n)
        if src_size is not None and (int(src_size[0]), int(src_size[1])) != (int(src.shape[2]), int(src.shape[1])):
            raise ValueError("src_size %r does not match src of shape %s" % (tuple(src_size), tuple(src.shape)))
        src_size = (int(src.shape[2]), int(src.shape[1]))
        sptr, sbytes = src.data_ptr(), src.numel()
        if out is None and stream is None and n > 0:
            out = torch.empty(tensor_shape(n, size, layout), dtype=getattr(torch, dtype), device=src.device)   # (written on torch's current stream, as src was)
    wd = warp_desc(src_size, warp_filter)
    marr = make_maps(maps, n)
    f = None if fill is None else tensor_fill(fill, fill_domain)
    stage = _WarpStage(lib, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: getattr(lib, lib_call)(sptr, sbytes, C.byref(wd), marr, f, desc, n_, ptr, room, stream_)
    out = _to_tensor(stage, call, size, None, dtype, layout, mean, std, scale, bias, 0, out, stream)
    return stage.tensor_to_host() if to_host else out


def tensor_warp(src, size, maps, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", dtype="float16", layout="NCHW", mean=None,
                std=None, scale=None, bias=None, out=None, stream=None, to_host=False):
    """asynchronous: the warp stage alone (hipdec_tensor_warp) over n = len(maps) dense 8-bit RGB samples in device memory: a uint8 torch.Tensor of shape
    (n, src_height, src_width, 3), or a DeviceBuffer of n * src_height * src_width * 3 bytes with src_size = (src_width, src_height).  Sample e goes through
    PIL.Image.transform(size, AFFINE, maps[e], warp_filter, fillcolor=fill) bit for bit and is normalised as to_tensor normalises; everything else as in
    Batch.to_tensor_warped.  A clip's T frames share one map by repeating it T times.  Returns `out` (to_host=True: the NumPy array, after waiting)."""
    return _tensor_map_stage("hipdec_tensor_warp", tensor_maps, src, size, maps, src_size, warp_filter, fill, fill_domain, dtype, layout, mean, std, scale, bias,
                             out, stream, to_host)


def tensor_project(src, size, maps, src_size=None, warp_filter=SCALE_BILINEAR, fill=0, fill_domain="component", dtype="float16", layout="NCHW", mean=None,
                   std=None, scale=None, bias=None, out=None, stream=None, to_host=False):
    """asynchronous: the projective stage alone (hipdec_tensor_project): tensor_warp with maps as Batch.to_tensor_projected takes them - sample e goes
    through PIL.Image.transform(size, PERSPECTIVE | QUAD, maps[e], warp_filter, fillcolor=fill) bit for bit.  Everything else as tensor_warp; dtype "uint8"
    with layout "NHWC" gives samples that tensor_warp, tensor_photo, tensor_augment, tensor_recipe and this call take again."""
    return _tensor_map_stage("hipdec_tensor_project", tensor_projections, src, size, maps, src_size, warp_filter, fill, fill_domain, dtype, layout, mean, std,
                             scale, bias, out, stream, to_host)


def _tensor_chain_stage(lib_call, make_chains, src, chains, src_size, dtype, layout, mean, std, scale, bias, out, stream, to_host):
    """tensor_photo and tensor_augment: the source, the chains, then the stage's call"""
    lib = _bind(load_library())
    chains = list(chains)
    n = len(chains)
    if isinstance(src, DeviceBuffer):
        if src_size is None:
            raise ValueError("a DeviceBuffer source needs src_size = (width, height)")
        sptr, sbytes = src.ptr, src.nbytes
    else:
        import torch
        if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8:
            raise TypeError("src must be a DeviceBuffer or a CUDA / HIP torch.Tensor of uint8")
        if src.dim() != 4 or src.shape[0] != n or src.shape[3] != 3 or not src.is_contiguous():
            raise ValueError("src must be contiguous with shape (%d, height, width, 3)" % n)
        if src_size is not None and (int(src_size[0]), int(src_size[1])) != (int(src.shape[2]), int(src.shape[1])):
            raise ValueError("src_size %r does not match src of shape %s" % (tuple(src_size), tuple(src.shape)))
        src_size = (int(src.shape[2]), int(src.shape[1]))
        sptr, sbytes = src.data_ptr(), src.numel()
        if out is None and stream is None and n > 0:
            out = torch.empty(tensor_shape(n, src_size, layout), dtype=getattr(torch, dtype), device=src.device)   # (written on torch's current stream, as src was)
    size = (int(src_size[0]), int(src_size[1]))
    pd = photo_desc(size)
    carr = make_chains(chains, n)
    carr = carr if isinstance(carr, tuple) else (carr,)   # (the recipe stage: the chains, the affine records, their number)
    stage = _WarpStage(lib, n)
    call = lambda h, desc, arr, n_, ptr, room, stream_: getattr(lib, lib_call)(sptr, sbytes, C.byref(pd), *carr, desc, n_, ptr, room, stream_)
    out = _to_tensor(stage, call, size, None, dtype, layout, mean, std, scale, bias, 0, out, stream)
    return stage.tensor_to_host() if to_host else out


def tensor_photo(src, chains, src_size=None, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None,
                 to_host=False):
    """asynchronous: the photometric stage alone (hipdec_tensor_photo) over n = len(chains) dense 8-bit RGB samples in device memory: a uint8 torch.Tensor
    of shape (n, height, width, 3), or a DeviceBuffer of n * height * width * 3 bytes with src_size = (width, height).  Sample e goes through chains[e] as
    in Batch.to_tensor_photo and is normalised as to_tensor normalises; the tensor has the samples' size.  dtype "uint8" with layout "NHWC" gives samples
    that tensor_warp and tensor_photo take again.  A clip's T frames share one chain by repeating it T times.  `out`: a DeviceBuffer, or a torch tensor on
    the current stream.  Returns `out` (to_host=True: the NumPy array, after waiting)."""
    return _tensor_chain_stage("hipdec_tensor_photo", photo_chains, src, chains, src_size, dtype, layout, mean, std, scale, bias, out, stream, to_host)


def tensor_augment(src, chains, src_size=None, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None,
                   to_host=False):
    """asynchronous: the augment stage alone (hipdec_tensor_augment): tensor_photo with chains as Batch.to_tensor_augmented takes them - up to
    AUGMENT_MAX_OPS operations, hue and Gaussian blur among them.  Everything else as tensor_photo; dtype "uint8" with layout "NHWC" gives samples that
    tensor_warp, tensor_photo and tensor_augment take again."""
    return _tensor_chain_stage("hipdec_tensor_augment", augment_chains, src, chains, src_size, dtype, layout, mean, std, scale, bias, out, stream, to_host)


def tensor_recipe(src, chains, src_size=None, dtype="float16", layout="NCHW", mean=None, std=None, scale=None, bias=None, out=None, stream=None,
                  to_host=False):
    """asynchronous: the recipe stage alone (hipdec_tensor_recipe): tensor_augment with chains as Batch.to_tensor_recipe takes them - affine steps with
    their own warp filter and fill among the operations.  Everything else as tensor_photo: `out` a DeviceBuffer, or a torch tensor on the current stream;
    dtype "uint8" with layout "NHWC" gives samples that tensor_warp, tensor_photo, tensor_augment and tensor_recipe take again."""
    return _tensor_chain_stage("hipdec_tensor_recipe", recipe_chains, src, chains, src_size, dtype, layout, mean, std, scale, bias, out, stream, to_host)


def clips_stats():
    """(launch sets built, their tracks, their frames, clip tensor calls, frames through the strided box kernel) since load"""
    lib = _bind(load_library())
    v = [C.c_uint64() for _ in range(5)]
    lib.hipdec_clips_stats(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def uniform_frames(frame_count, T, stride=1, start=0, pad="repeat_last"):
    """T frame indices start, start + stride, ... of a track of frame_count frames - the usual uniform sampling of a video loader.  Indices past the last
    frame: pad "repeat_last" clamps them to it, "loop" wraps them around, "error" raises ValueError."""
    frame_count, T, stride, start = int(frame_count), int(T), int(stride), int(start)
    if frame_count < 1 or T < 1 or stride < 1 or start < 0 or start >= frame_count:
        raise ValueError("uniform_frames: frame_count %d, T %d, stride %d, start %d" % (frame_count, T, stride, start))
    idx = [start + k * stride for k in range(T)]
    if pad == "repeat_last":
        return [min(i, frame_count - 1) for i in idx]
    if pad == "loop":
        return [i % frame_count for i in idx]
    if pad == "error":
        if idx[-1] >= frame_count:
            raise ValueError("uniform_frames: frame %d of a track of %d" % (idx[-1], frame_count))
        return idx
    raise ValueError("pad must be repeat_last, loop or error")


def clip_packed_layout(sizes, T, patch=0, merge=1, temporal_patch=1):
    """(offsets, tokens, total elements) of clips of T frames of the DISPLAYED sizes (width, height) packed back to back in entry order
    (hipdec_clip_packed_layout; host only): tokens[e] = (T / temporal_patch) * (width / patch) * (height / patch), 0 for dense clips."""
    lib = _bind(load_library())
    n = len(sizes)
    ws, hs = (C.c_int * n)(*(int(s[0]) for s in sizes)), (C.c_int * n)(*(int(s[1]) for s in sizes))
    offs, toks, total = (C.c_uint64 * n)(), (C.c_uint32 * n)(), C.c_uint64()
    pt = TensorPatches(int(patch), int(merge))
    cd = ClipDesc(int(T), 0, int(temporal_patch), 0)
    if lib.hipdec_clip_packed_layout(C.byref(cd), C.byref(pt), ws, hs, n, offs, toks, C.byref(total)) != 0:
        raise ValueError("clip_packed_layout: %s" % lib.hipdec_last_error().decode())
    return list(offs), list(toks), total.value


class _BorrowedBatch(Batch):
    """Clips.batch: the launch set of a Clips object as a Batch.  Not owned - free() and __del__ do nothing, run() is refused by the library - and
    valid as long as the Clips object is (Clips.free() clears the handle)."""

    def __init__(self, lib, handle, n):
        self._lib, self._h, self.n = lib, C.c_void_p(handle), n

    def free(self):
        pass

    def __del__(self):
        pass


class Clips:
    """The samples of several sequence tracks decoded by ONE launch set, every picture resident in device memory, and video tensors from them
    (hipdec_clips_*).  tracks: a list of tracks, each a list of samples (bytes) in decoding order, in the framing of HipDecoder.push_data; a track's first
    sample carries the parameter sets.  The FRAMES of a track are its output pictures in output order."""

    def __init__(self, tracks, max_image_size_pixels=0):
        self._lib = _bind(load_library())
        self._keep = [bytes(s) for t in tracks for s in t]
        n = len(self._keep)
        counts = (C.c_int * max(len(tracks), 1))(*[len(t) for t in tracks])
        arr = (C.c_char_p * max(n, 1))(*self._keep)
        sizes = (C.c_size_t * max(n, 1))(*[len(s) for s in self._keep])
        self._h = C.c_void_p()
        check(self._lib.hipdec_clips_create(C.byref(self._h), len(tracks), counts, arr, sizes, int(max_image_size_pixels)))
        self.n_tracks = self._lib.hipdec_clips_track_count(self._h)
        bh = self._lib.hipdec_clips_batch(self._h)
        self.batch = _BorrowedBatch(self._lib, bh, self._lib.hipdec_batch_count(bh))

    def run(self, stream=None):
        check(self._lib.hipdec_clips_run(self._h, stream))

    def status(self):
        check(self._lib.hipdec_clips_status(self._h))

    def frame_count(self, t):
        n = self._lib.hipdec_clips_frame_count(self._h, t)
        if n < 0:
            check(n)
        return n

    def frame(self, t, f):
        """{"item", "sample", "poc", "sequence"} and the picture's info fields"""
        cf = ClipFrame()
        check(self._lib.hipdec_clips_frame(self._h, t, f, C.byref(cf)))
        d = _info_dict(cf.info)
        d.update(item=cf.item, sample=cf.sample, poc=cf.poc, sequence=cf.sequence)
        return d

    def info(self, i=0):
        return self.batch.info(i)

    def planes(self, t, f):
        d = self.frame(t, f)
        dt = np.uint16 if d["bit_depth_luma"] > 8 else np.uint8
        out = []
        for c in range(3 if d["chroma_format_idc"] else 1):
            w, h = (d["width"], d["height"]) if c == 0 else (d["chroma_width"], d["chroma_height"])
            a = np.empty((h, w), dt)
            check(self._lib.hipdec_clips_read_plane(self._h, t, f, c, a.ctypes.data, w * a.itemsize))
            out.append(a)
        return out

    def _frames_array(self, frames, n, T):
        flat = [int(f) for clip in frames for f in clip] if len(frames) and hasattr(frames[0], "__len__") else [int(f) for f in frames]
        if len(flat) != n * T:
            raise ValueError("%d frame indices for %d clips of %d frames" % (len(flat), n, T))
        return (C.c_int * len(flat))(*flat)

    def to_tensor(self, size, T, entries, frames, order="TCHW", dtype="float16", mean=None, std=None, scale=None, bias=None, filter=1, orientations=None,
                  out=None, stream=None):
        """asynchronous: one clip of T frames per entry as ONE dense tensor (hipdec_clips_to_tensor).  entries: (track, left, top, width, height[, flip])
        tuples - one window and one flip for the whole clip; frames: T frame indices of the entry's track per entry (uniform_frames()), nested or flat.
        order: "TCHW" (N, T, 3, H, W), "CTHW" (N, 3, T, H, W) or "THWC" (N, T, H, W, 3).  Everything else as Batch.to_tensor; each frame is what
        Clips.batch.to_tensor(..., orientations=) writes for the frame's item."""
        if order not in CLIP_ORDERS:
            raise ValueError("order must be one of %s" % sorted(CLIP_ORDERS))
        T = int(T)
        co, layout = CLIP_ORDERS[order]
        n = len(entries)
        W, H = int(size[0]), int(size[1])
        shape = {"TCHW": (n, T, 3, H, W), "CTHW": (n, 3, T, H, W), "THWC": (n, T, H, W, 3)}[order]
        cd = ClipDesc(T, co, 0, 0)
        fr = self._frames_array(frames, n, T)
        codes = None if orientations is None else _orientation_array(orientations, n)
        call = lambda h, desc, arr, n_, ptr, room, s: self._lib.hipdec_clips_to_tensor(h, desc, C.byref(cd), arr, fr, codes, n_, ptr, room, s)
        return self._go(call, (W, H), shape, entries, dtype, layout, mean, std, scale, bias, filter, out, stream)

    def _go(self, call, size, shape, entries, dtype, layout, mean, std, scale, bias, filter, out, stream):
        d0 = self.batch.info(0)
        max_value = (1 << d0["bit_depth_luma"]) - 1 if (dtype != "uint8" and d0["bit_depth_luma"] > 8) else 255
        sc, bi = tensor_scale_bias(mean, std, scale, bias, max_value)
        desc = tensor_desc(size, dtype, layout, filter, sc, bi)
        item = np.dtype(_TENSOR_NUMPY[dtype]).itemsize
        nbytes = int(np.prod(shape)) * item
        arr = tensor_entries(entries)
        host_wait = False
        if out is None:
            torch = _torch_gpu()
            out = torch.empty(shape, dtype=getattr(torch, dtype), device="cuda") if torch is not None else DeviceBuffer(max(nbytes, 1))
        if isinstance(out, DeviceBuffer):
            ptr, room = out.ptr, out.nbytes
        else:
            import torch
            if not isinstance(out, torch.Tensor) or not out.is_cuda:
                raise TypeError("out must be a DeviceBuffer or a CUDA / HIP torch.Tensor")
            if len(shape) == 1:   # token sequences and packed clips: a 1-D tensor that may be longer than the clips (gaps and a tail stay as they are)
                if out.dim() != 1 or out.numel() < shape[0]:
                    raise ValueError("out must be a 1-D tensor of at least %d elements" % shape[0])
            elif tuple(out.shape) != tuple(shape):
                raise ValueError("out has shape %s, the tensor has %s" % (tuple(out.shape), tuple(shape)))
            if out.dtype != getattr(torch, dtype):
                raise ValueError("out has dtype %s, the tensor has %s" % (out.dtype, dtype))
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            ptr, room = out.data_ptr(), out.numel() * item
            if stream is None:
                ts = torch.cuda.current_stream(out.device)
                stream = ts.cuda_stream or None
                if stream is None:   # (torch's legacy default stream: ordered on the host, as in Batch.to_tensor)
                    ts.synchronize()
                    host_wait = True
        check(call(self._h, C.byref(desc), arr, len(entries), ptr, room, stream))
        if host_wait:
            check(self._lib.hipdec_stream_synchronize(None))
        self._tensor = (out, tuple(shape), _TENSOR_NUMPY[dtype], stream)
        return out

    def to_tokens(self, sizes, T, entries, frames, patch, merge=1, temporal_patch=1, layout="NCHW", order="TCHW", dtype="float16", mean=None, std=None,
                  scale=None, bias=None, filter=1, orientations=None, offsets=None, out=None, stream=None):
        """asynchronous: one clip per entry at its OWN displayed size sizes[e] = (width, height) into one 1-D output (hipdec_clips_to_tensor_packed): token
        sequences with a temporal patch (patch P >= 1: a token is 3 * temporal_patch * P * P elements, (c, k, py, px) for "NCHW" and (k, py, px, c) for
        "NHWC"; merge 2 with temporal_patch 2 is the order of Qwen2-VL's video tokens), or dense clips in `order` (patch 0).  offsets None: back to back
        (clip_packed_layout()).  Returns (out, offsets, grids), grids[e] = (T / temporal_patch, height / P, width / P) for patches, None for dense clips."""
        T, patch, merge, Tp = int(T), int(patch), int(merge), int(temporal_patch)
        n = len(entries)
        sizes = [(int(w), int(h)) for w, h in sizes]
        if len(sizes) != n:
            raise ValueError("%d sizes for %d entries" % (len(sizes), n))
        if patch == 0 and order != "TCHW":
            if order not in CLIP_ORDERS:
                raise ValueError("order must be one of %s" % sorted(CLIP_ORDERS))
            co, layout = CLIP_ORDERS[order]
        else:
            co = 0
        if offsets is None:
            offsets, _, total = clip_packed_layout(sizes, T, patch, merge, Tp)
        else:
            offsets = [int(o) for o in offsets]
            if len(offsets) != n:
                raise ValueError("%d offsets for %d entries" % (len(offsets), n))
            total = max(o + 3 * T * w * h for o, (w, h) in zip(offsets, sizes))
        samples = (TensorSample * n)(*(TensorSample(w, h, o) for (w, h), o in zip(sizes, offsets)))
        pt = TensorPatches(patch, merge)
        cd = ClipDesc(T, co, Tp, 0)
        fr = self._frames_array(frames, n, T)
        codes = None if orientations is None else _orientation_array(orientations, n)
        call = lambda h, desc, arr, n_, ptr, room, s: self._lib.hipdec_clips_to_tensor_packed(h, desc, C.byref(cd), arr, fr, codes, samples, C.byref(pt), n_, ptr,
                                                                                              room, s)
        out = self._go(call, (0, 0), (total,), entries, dtype, layout, mean, std, scale, bias, filter, out, stream)
        grids = [(T // max(Tp, 1), h // patch, w // patch) for w, h in sizes] if patch else None
        return out, offsets, grids

    def tensor_to_host(self):
        """the last to_tensor() / to_tokens() result as a NumPy array of its shape (bfloat16 as uint16 bit patterns); waits for its stream"""
        out, shape, dt, stream = self._tensor
        check(self._lib.hipdec_stream_synchronize(stream))
        if isinstance(out, DeviceBuffer):
            return out.to_numpy(shape, dt)
        import torch
        t = out.view(torch.int16) if dt == np.uint16 else out
        a = (t[:shape[0]] if len(shape) == 1 else t).cpu().numpy()
        return a.view(np.uint16) if dt == np.uint16 else a

    def free(self):
        if self._h:
            self._lib.hipdec_clips_free(self._h)
            self._h = C.c_void_p()
            self.batch._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
