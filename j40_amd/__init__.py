"""j40_amd -- Python host-side mirror of the j40 C API on top of libj40hip.so (MI355X / gfx950).

Thin ctypes plumbing only: the product is build/libj40hip.so (C++ host parser + HIP kernels). The
module fails loudly when the library is missing -- there is no Python or CPU fallback for the hot
path. Function names mirror the reference's public API (j40.h:233-272):

    img = j40_amd.from_memory(data)      # j40_from_memory
    img.output_format(J40_RGBA, J40_U8X4)
    if img.next_frame():                 # j40_next_frame
        rgba = img.frame_pixels_u8x4()   # j40_current_frame + j40_frame_pixels_u8x4 (numpy view copy)
    # 16-bit RGBA (J40_U16X4): img.output_format(J40_RGBA, J40_U16X4) before next_frame, then img.frame_pixels_u16x4()
    img.error(), img.error_string(); img.free()

`Frame` exposes the thin C-ABI of include/j40hip.h (parse / upload / decode on a stream / status /
stage dumps) for the parity tests, bench.py and the multi-GPU driver.
"""
import weakref
import ctypes as C
import os
import numpy as np

J40_RGBA = 0x1755
J40_U8X4 = 0x0F33
J40_U16X4 = 0x0F35
PARSE_LF_ONLY = 2   # J40HIP_PARSE_LF_ONLY (include/j40hip.h): the LF preview's parse
PARSE_YCBCR = 4     # J40HIP_PARSE_YCBCR: YCbCr frames are asked for (a subsampled one is parsed instead of refused)
PARSE_SPLINES = 1024   # J40HIP_PARSE_SPLINES / J40HIP_SEQ_SPLINES: splines are asked for (a frame with has_splines is parsed and its splines drawn instead of "TODO"); j40hip_sequence_open takes it too
PARSE_NOISE = 256   # J40HIP_PARSE_NOISE: photon noise is asked for (a frame with has_noise is parsed and its noise added instead of "TODO"); j40hip_sequence_open takes it too
PARSE_UPSAMPLING = 512   # J40HIP_PARSE_UPSAMPLING: upsampling is asked for (custom weights and a frame coded at 1:2, 1:4 or 1:8 are parsed and served instead of "TODO"); J40HIP_SEQ_UPSAMPLING is the same bit
PARSE_WIDE = 8      # J40HIP_PARSE_WIDE: wide Modular frames are asked for (an image with 32-bit Modular buffers is parsed instead of "fm32")

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("J40HIP_LIB") or os.path.join(_ROOT, "build", "libj40hip.so")
_lib = None


class J40Error(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        super().__init__("j40 error %r %s" % (code, where))


def err4(code):
    return "".join(chr((code >> s) & 0xFF) for s in (24, 16, 8, 0)) if code else ""


class _Image(C.Structure):
    class _U(C.Union):
        _fields_ = [("inner", C.c_void_p), ("err", C.c_uint32), ("saved_errno", C.c_int)]
    _fields_ = [("magic", C.c_uint32), ("u", _U)]


class _FrameHandle(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("reserved", C.c_uint32), ("inner", C.c_void_p)]


class _Pixels(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride_bytes", C.c_int32), ("data", C.c_void_p)]


class _PixelsU16(C.Structure):
    """j40_pixels_u16x4 (include/j40.h): the same layout as j40_pixels_u8x4"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride_bytes", C.c_int32), ("data", C.c_void_p)]


# j40hip_output_alloc (include/j40hip.h): (ctx, width, height, *stride_bytes) -> host memory for the pixels
OUTPUT_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_size_t))


def lib():
    """loads build/libj40hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libj40hip.so is missing at %s: run `make lib` (or __graft_entry__.build())" % LIB_PATH)
    # PyTorch wheels bundle their own libamdhip64; a process that loads both that copy and /opt/rocm's ends up with
    # two HIP runtimes of which only the first sees the GPU. Let torch (the plumbing for device buffers, streams and
    # torch.distributed) load first when it is installed, so that libj40hip.so binds to the runtime already there.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, i32, i64, sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_int64, C.c_size_t
    sigs = {
        "j40_error": (u32, [vp]), "j40_error_string": (C.c_char_p, [vp]),
        "j40_from_memory": (u32, [vp, vp, sz, vp]), "j40_from_file": (u32, [vp, C.c_char_p]),
        "j40_output_format": (u32, [vp, i32, i32]), "j40_next_frame": (C.c_int, [vp]),
        "j40_current_frame": (_FrameHandle, [vp]), "j40_frame_pixels_u8x4": (_Pixels, [vp, i32]),
        "j40_row_u8x4": (vp, [_Pixels, i32]), "j40_free": (None, [vp]),
        "j40_frame_pixels_u16x4": (_PixelsU16, [vp, i32]), "j40_row_u16x4": (vp, [_PixelsU16, i32]),
        "j40hip_frame_set_output_format": (u32, [vp, i32]), "j40hip_frame_output_format": (i32, [vp]),
        "j40hip_kat_device_srgb_u16": (u32, [vp, sz, i32, vp]),
        "j40hip_frame_parse": (vp, [vp, sz, C.c_int, C.POINTER(u32)]), "j40hip_frame_free": (None, [vp]),
        "j40hip_frame_parse_ex": (vp, [vp, sz, C.c_int, u32, C.POINTER(u32)]),
        "j40hip_frame_info": (None, [vp, vp]), "j40hip_frame_codestream_size": (sz, [vp]), "j40hip_frame_num_sections": (i64, [vp]),
        "j40hip_frame_lf_group_info": (None, [vp, i64, vp]), "j40hip_frame_lf_group_plane": (C.c_int, [vp, i64, C.c_int, vp]),
        "j40hip_frame_varblocks": (None, [vp, i64, vp, vp]), "j40hip_frame_llf": (None, [vp, i64, C.c_int, vp]),
        "j40hip_frame_dq_matrix": (i32, [vp, C.c_int, vp]), "j40hip_frame_order": (i32, [vp, C.c_int, C.c_int, C.c_int, vp]),
        "j40hip_frame_block_ctx_map": (i32, [vp, vp]), "j40hip_frame_global_plane": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32), C.POINTER(i32)]),
        "j40hip_kat_natural_order": (i32, [i32, i32, vp]), "j40hip_kat_library_dq_matrix": (i32, [C.c_int, vp]),
        "j40hip_kat_forward_llf": (None, [vp, i32, i32]), "j40hip_kat_half_secant": (C.c_float, [C.c_int]),
        "j40hip_kat_lf2llf_scale": (C.c_float, [C.c_int]),
        "j40hip_device_count": (C.c_int, []), "j40hip_frame_upload": (u32, [vp, C.c_int]),
        "j40hip_frame_set_group_range": (u32, [vp, i64, i64]), "j40hip_frame_decode": (u32, [vp, vp, sz, vp]),
        "j40hip_frame_status": (u32, [vp]), "j40hip_frame_decode_to_host": (u32, [vp, vp, sz]), "j40hip_frame_two_phase_sections": (C.c_int32, [vp]),
        "j40hip_frame_read_coeffs": (u32, [vp, i64, C.c_int, vp]), "j40hip_frame_read_plane_i16": (u32, [vp, C.c_int, vp]),
        "j40hip_frame_decode_timed": (u32, [vp, vp, sz, vp, vp]), "j40hip_frame_force_dense": (None, [vp, C.c_int]),
        "j40hip_kat_device_srgb_u8": (u32, [vp, sz, vp]),
        "j40hip_batch_create": (vp, [vp, i64, C.POINTER(u32)]), "j40hip_batch_free": (None, [vp]),
        "j40hip_batch_decode": (u32, [vp, vp, vp, vp]), "j40hip_batch_decode_timed": (u32, [vp, vp, vp, vp, vp]),
        "j40hip_batch_decode_recorded": (u32, [vp, vp, vp, vp, i32]), "j40hip_batch_elapsed": (u32, [vp, i32, vp]), "j40hip_batch_wait_stage": (u32, [vp, i32, i32, vp]),
        "j40hip_batch_reset": (u32, [vp, vp, i64]), "j40hip_frame_section_sizes": (i64, [vp, vp]), "j40hip_frame_coop_sections": (i32, [vp, vp]), "j40hip_frame_quad_sections": (i32, [vp]), "j40hip_frame_split_sections": (i32, [vp]), "j40hip_frame_lf_bundle": (sz, [vp, vp, sz, vp]), "j40hip_frame_parse_on": (vp, [vp, sz, C.c_int, u32, C.c_int, vp, vp]), "j40hip_frame_lf_on_device": (C.c_int, [vp]), "j40hip_frame_from_lf_bundle": (vp, [vp, sz, vp]),
        "j40hip_frame_upload_on": (u32, [vp, C.c_int, vp]), "j40hip_thread_release": (None, []), "j40hip_shutdown": (None, []),
        "j40hip_frame_status_begin": (u32, [vp, vp]), "j40hip_frame_status_end": (u32, [vp]), "j40hip_frame_mark_idle": (None, [vp]),
        "j40hip_frame_after_frame_status": (u32, [vp]),
        "j40hip_pipeline_create": (vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(u32)]), "j40hip_pipeline_free": (None, [vp]), "j40hip_pipeline_create_ex": (vp, [C.c_int, C.c_int, C.c_int, C.c_int, u32, C.POINTER(u32)]), "j40hip_pipeline_lf_device_frames": (i64, [vp]),
        "j40hip_pipeline_submit": (u32, [vp, vp, sz, vp, sz, C.c_int, C.POINTER(i64)]), "j40hip_pipeline_drain": (u32, [vp]),
        "j40hip_pipeline_run": (u32, [vp, vp, sz, OUTPUT_ALLOC, vp]), "j40hip_pipeline_set_max_wait_ms": (None, [vp, C.c_double]),
        "j40hip_stage_dump_create": (vp, [vp, sz, C.c_int, C.c_int, C.POINTER(u32)]), "j40hip_stage_dump_free": (None, [vp]), "j40hip_stage_dump_info": (None, [vp, vp]),
        "j40hip_stage_dump_lf_group_info": (C.c_int, [vp, i64, vp]), "j40hip_stage_dump_plane": (C.c_int, [vp, i64, C.c_int, vp]),
        "j40hip_stage_dump_varblocks": (C.c_int, [vp, i64, vp, vp, vp]), "j40hip_stage_dump_llf": (C.c_int, [vp, i64, C.c_int, vp]),
        "j40hip_stage_dump_group_blocks": (i64, [vp, i64, vp, i64]), "j40hip_stage_dump_sorted_varblocks": (i64, [vp, vp, vp, vp, i64]), "j40hip_stage_dump_rgba": (C.c_int, [vp, vp]),
        "j40hip_copy_engine": (C.c_int, [C.c_int, vp, vp]),
        "j40hip_sequence_open": (vp, [vp, sz, C.c_int, u32, C.POINTER(u32)]), "j40hip_sequence_free": (None, [vp]),
        "j40hip_sequence_num_frames": (i64, [vp]), "j40hip_sequence_num_shown": (i64, [vp]), "j40hip_sequence_frame_info": (None, [vp, i64, vp]),
        "j40hip_sequence_frame": (vp, [vp, i64, C.POINTER(u32)]), "j40hip_sequence_upload": (u32, [vp, C.c_int]),
        "j40hip_sequence_set_output_format": (u32, [vp, i32]), "j40hip_sequence_next": (u32, [vp, vp, sz, vp]),
        "j40hip_sequence_next_to_host": (u32, [vp, vp, sz]), "j40hip_sequence_rewind": (None, [vp]), "j40hip_sequence_status": (u32, [vp, C.POINTER(i64)]),
        "j40hip_kat_device_compose": (u32, [vp, sz, vp, sz, vp, sz, i32, i32, i32, i32, i32, i32, u32, u32, i32, vp]),
        "j40hip_sequence_frame_blend": (None, [vp, i64, vp]),
        "j40hip_sequence_frame_lf": (None, [vp, i64, vp]), "j40hip_sequence_read_lf_slot": (u32, [vp, i32, i32, vp]),
        "j40hip_set_upsampling_defaults": (u32, [C.c_int, vp, C.c_int]), "j40hip_frame_upsampling": (u32, [vp, vp, vp, vp]),
        "j40hip_frame_coded_size": (None, [vp, vp, vp]), "j40hip_frame_upsample_ms": (C.c_float, [vp]),
        "j40hip_kat_upsampling_kernel": (u32, [i32, vp, vp]),
        "j40hip_kat_device_upsample": (u32, [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp]),
        "j40hip_kat_host_upsample": (u32, [vp, i32, i32, i32, vp, i32, i32, vp, C.c_int]),
        "j40hip_frame_noise": (C.c_int, [vp, vp, vp]), "j40hip_frame_noise_launches": (i64, [vp]), "j40hip_frame_noise_ms": (None, [vp, vp]),
        "j40hip_frame_splines": (C.c_int, [vp, vp, vp]), "j40hip_frame_spline": (u32, [vp, i64, vp, vp, vp, i64, vp]),
        "j40hip_frame_spline_segments": (i64, [vp, vp, i64]), "j40hip_frame_spline_bins": (None, [vp, vp]),
        "j40hip_frame_spline_launches": (i64, [vp]), "j40hip_frame_spline_ms": (C.c_float, [vp]),
        "j40hip_kat_device_splines": (u32, [vp, i32, i32, vp, i64, vp, vp, vp]),
        "j40hip_kat_device_noise": (u32, [vp, i32, i32, i32, vp, C.c_float, C.c_float, u32, u32, vp, vp, vp]),
        "j40hip_sequence_frame_patches": (None, [vp, i64, vp]), "j40hip_sequence_frame_patch": (u32, [vp, i64, i64, vp]),
        "j40hip_sequence_ref_slot_size": (u32, [vp, i32, vp, vp]), "j40hip_sequence_read_ref_slot": (u32, [vp, i32, i32, vp]),
        "j40hip_kat_device_patches": (u32, [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp]),
        "j40hip_kat_device_blend": (u32, [vp, sz, vp, sz, vp, sz, i32, i32, i32, i32, i32, i32, u32, u32, i32, i32, i32, vp]),
        "j40hip_frame_restoration": (None, [vp, vp]), "j40hip_frame_set_restoration": (None, [vp, C.c_int]), "j40hip_frame_sharpness": (C.c_int, [vp, i64, vp]),
        "j40hip_frame_set_alpha": (u32, [vp, C.c_int]), "j40hip_frame_alpha": (None, [vp, vp]),
        "j40hip_frame_set_ycbcr": (u32, [vp, C.c_int]), "j40hip_frame_ycbcr": (None, [vp, vp]), "j40hip_frame_read_ycbcr": (u32, [vp, C.c_int, vp]),
        "j40hip_frame_wide": (None, [vp, vp]), "j40hip_frame_read_plane_i32": (u32, [vp, C.c_int, vp]),
        "j40hip_kat_device_ycbcr_tail": (u32, [vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "j40hip_frame_set_modular_xyb": (u32, [vp, C.c_int]), "j40hip_frame_modular_xyb": (None, [vp, vp]),
        "j40hip_kat_device_modular_xyb": (u32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, sz, vp, vp]),
        "j40hip_kat_device_modular_xyb_launch": (u32, [i32, vp, i32, i32, i32, vp, vp, i32, i32, vp, sz, vp, vp]),
        "j40hip_kat_device_colour_frame": (sz, [vp, i32, vp, sz]),
        "j40hip_frame_set_colour": (u32, [vp, C.c_int]), "j40hip_frame_colour": (None, [vp, vp]), "j40hip_frame_colour_encoding": (None, [vp, vp]),
        "j40hip_colour_gamut_matrix": (u32, [vp, vp, vp]),
        "j40hip_colour_table": (u32, [vp, C.c_float, vp, sz, vp]),
        "j40hip_kat_device_colour_tail": (u32, [vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, sz, vp]),
        "j40hip_frame_set_region": (u32, [vp, i32, i32, i32, i32]), "j40hip_frame_region": (None, [vp, vp]),
        "j40hip_frame_set_scale": (u32, [vp, i32]), "j40hip_frame_scale": (None, [vp, vp]), "j40hip_pipeline_set_scale": (u32, [vp, i32]),
        "j40hip_kat_device_downscale": (u32, [vp, sz, vp, sz, i32, i32, i32, i32, vp]),
        "j40hip_frame_set_orientation": (u32, [vp, C.c_int]), "j40hip_frame_orientation": (None, [vp, vp]), "j40hip_frame_orient_rect": (u32, [vp, C.c_int, vp, vp]),
        "j40hip_kat_device_orient": (u32, [vp, sz, vp, sz, i32, i32, i32, i32, vp]),
        "j40hip_kat_device_alpha_merge": (u32, [vp, sz, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "j40hip_frame_read_xyb": (u32, [vp, C.c_int, vp]), "j40hip_frame_restoration_ms": (C.c_float, [vp]),
        "j40hip_kat_device_restoration": (u32, [vp, i32, i32, vp, vp, vp, C.c_int, C.c_int, vp]),
        "j40hip_frame_lf_end": (i64, [vp]), "j40hip_frame_lf_size": (None, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "j40hip_frame_lf_plane": (u32, [vp, C.c_int, vp]), "j40hip_frame_colour_consts": (None, [vp, vp]), "j40hip_frame_lf_dequant": (None, [vp, vp]),
        "j40hip_frame_decode_lf": (u32, [vp, vp, sz, vp]), "j40hip_frame_decode_lf_to_host": (u32, [vp, vp, sz]),
        "j40hip_frames_decode_lf": (u32, [vp, i64, vp, vp, vp]), "j40hip_frame_read_lf": (u32, [vp, C.c_int, vp]),
        "j40hip_pipeline_result": (u32, [vp, i64]), "j40hip_pipeline_stats": (None, [vp, vp]), "j40hip_pipeline_stats_ex": (None, [vp, vp]), "j40hip_pipeline_lf_stats": (None, [vp, vp]), "j40hip_pipeline_reset_stats": (None, [vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)  # AttributeError = the library does not export what include/*.h declares
        fn.restype = res
        fn.argtypes = args
    L._declared = sorted(sigs)
    _lib = L
    return L


def device_count():
    return lib().j40hip_device_count()


def copy_engine(device=0):
    """j40hip_copy_engine: the SDMA engine the pipeline's copies back to host memory go to on `device` (-1: hipMemcpyAsync), the measured
    device-to-host GB/s per engine and the runtime's {free, recommended} masks"""
    import numpy as np
    rates = np.zeros(16, np.float64); masks = np.zeros(3, np.uint32)
    e = lib().j40hip_copy_engine(device, rates.ctypes.data, masks.ctypes.data)
    return {"engine": e, "d2h_gb_per_s_per_engine": {str(i): round(float(r), 1) for i, r in enumerate(rates) if r != 0}, "engines_free_mask": hex(int(masks[0])), "engines_recommended_mask": hex(int(masks[1])), "upload_engines_mask": hex(int(masks[2]))}


def shutdown():
    """j40hip_shutdown: stops and joins the library's service threads and gives cached device memory, pooled events and cached tables
    back. Optional; every Frame / Batch / Pipeline of the process must have been closed."""
    if _lib is not None:
        _lib.j40hip_shutdown()


class Image:
    """mirror of a j40_image handle and the public API calls on it"""

    def __init__(self):
        self._img = _Image()
        self._buf = None
        self._live = False

    def error(self):
        return err4(lib().j40_error(C.byref(self._img)))

    def error_string(self):
        return lib().j40_error_string(C.byref(self._img)).decode()

    def output_format(self, channel=J40_RGBA, fmt=J40_U8X4):
        return err4(lib().j40_output_format(C.byref(self._img), channel, fmt))

    def next_frame(self):
        return bool(lib().j40_next_frame(C.byref(self._img)))

    def frame_pixels_u8x4(self, channel=J40_RGBA):
        """returns a numpy copy [height, width, 4] of the rendered frame (or of the error placeholder)"""
        L = lib()
        fr = L.j40_current_frame(C.byref(self._img))
        px = L.j40_frame_pixels_u8x4(C.byref(fr), channel)
        rows = np.ctypeslib.as_array(C.cast(px.data, C.POINTER(C.c_uint8)), shape=(px.height, px.stride_bytes))
        return rows[:, : px.width * 4].reshape(px.height, px.width, 4).copy(), px.stride_bytes, px.data

    def frame_pixels_u16x4(self, channel=J40_RGBA):
        """the 16-bit counterpart (J40_U16X4): a uint16 numpy copy [height, width, 4], the stride in bytes, the data pointer"""
        L = lib()
        fr = L.j40_current_frame(C.byref(self._img))
        px = L.j40_frame_pixels_u16x4(C.byref(fr), channel)
        rows = np.ctypeslib.as_array(C.cast(px.data, C.POINTER(C.c_uint16)), shape=(px.height, px.stride_bytes // 2))
        return rows[:, : px.width * 4].reshape(px.height, px.width, 4).copy(), px.stride_bytes, px.data

    def free(self):
        if self._live:
            lib().j40_free(C.byref(self._img))
            self._live = False


def from_memory(data: bytes) -> Image:
    img = Image()
    img._buf = C.create_string_buffer(data, len(data))  # borrowed by the library until free()
    lib().j40_from_memory(C.byref(img._img), img._buf, len(data), None)
    img._live = True
    return img


def from_file(path: str) -> Image:
    img = Image()
    lib().j40_from_file(C.byref(img._img), path.encode())
    img._live = True
    return img


def decode(data: bytes, fmt=J40_U8X4, alpha=False, scale=0, ycbcr=False, orient=False, wide=False, lf_frames=False, modular_xyb=False, colour=False, patches=False, blend=False, noise=False, upsampling=False, splines=False):
    """whole path through the public API; returns (err4, rgba ndarray or None): uint8 [h, w, 4], or uint16 with fmt=J40_U16X4.
    scale=1 / 2: the 1:2 / 1:4 image, ceil(h / s) x ceil(w / s), every sample the rounded mean of its cell of the full decode
    (Frame.set_scale); like alpha=True it goes through the thin C-ABI on device 0.
    The public API writes a VarDCT frame's alpha as the environment says (J40HIP_ALPHA=1 keeps it, else A is opaque like the
    reference's). alpha=True keeps it for this call whatever the environment says: the frame goes through the thin C-ABI with
    Frame.set_alpha(1) on device 0 -- "TODO" / "Ual?" where that refuses (Frame.set_alpha).
    ycbcr=True: a YCbCr VarDCT frame (a recompressed JPEG) is served for this call whatever J40HIP_YCBCR says (Frame.set_ycbcr(1)),
    likewise through the thin C-ABI on device 0; "TODO" for what that does not serve.
    orient=True: the picture in the orientation the stream carries (Frame.set_orientation(1)), [ow, oh] swapped for orientations 5 to
    8, whatever J40HIP_ORIENT says; likewise through the thin C-ABI on device 0.
    wide=True: an image with 32-bit Modular buffers (every 16-bit lossless image) is served for this call whatever J40HIP_WIDE says
    (PARSE_WIDE), likewise through the thin C-ABI on device 0; its VarDCT frames are "TODO".
    lf_frames=True: a still whose LF image is a frame of its own (LF frames, then the frame with use_lf_frame) is served for this call
    whatever J40HIP_LFFRAME says: through a Sequence on device 0, the first displayed canvas. It combines with fmt, scale and orient
    ("TODO" with the other switches): the playback fills the LF slots at full size, then the main frame's own handle -- which keeps
    its LF source -- is decoded once more at the scale and / or in the orientation, as any frame is (Frame.set_scale,
    Frame.set_orientation; a refusal where the shown frame is not a full-canvas frame with use_lf_frame). A stream that is no
    sequence is decoded as without it.
    modular_xyb=True: a Modular frame of an XYB image goes through the XYB colour tail for this call whatever J40HIP_MODULAR_XYB says
    (Frame.set_modular_xyb(1); "Umx?" for a frame the rule does not apply to), through the thin C-ABI on device 0. With lf_frames=True
    the sequence is opened with both switches, which serves a Modular LF frame.
    colour=True: an XYB image is rendered in the colour space its header signals for this call whatever J40HIP_COLOUR says
    (Frame.set_colour(1); "Ucs?" for what that refuses), through the thin C-ABI on device 0; with lf_frames=True the sequence is opened
    with the switch.
    patches=True: a stream with reference-only frames and patch dictionaries is served for this call whatever J40HIP_PATCHES says:
    through a Sequence on device 0 opened with the switch (Sequence's patches=), the first displayed canvas. It combines with
    modular_xyb=, colour=, lf_frames= and blend= (Sequence's blend=, which only this route takes), which open the sequence with theirs,
    and with fmt and scale (the shown frame's own handle decoded once more at the scale, as with lf_frames=True: a full-canvas frame with
    patches takes one); "TODO" with orient= unless lf_frames= is given too.
    noise=True: a frame with photon noise (has_noise) is served for this call whatever J40HIP_NOISE says (PARSE_NOISE; PARITY UNPINNED),
    through the thin C-ABI on device 0; it combines with every switch above (a sequence is opened with it).
    upsampling=True: a frame coded at 1:2, 1:4 or 1:8 (and custom upsampling weights) is served for this call whatever J40HIP_UPSAMPLING
    says (PARSE_UPSAMPLING; PARITY UNPINNED), through the thin C-ABI on device 0: the picture has the shown size. It combines with fmt,
    scale, orient, modular_xyb (which a Modular frame needs) and colour; "TODO" with alpha=True and for every frame of a sequence.
    splines=True: a frame with splines (has_splines) is served for this call whatever J40HIP_SPLINES says (PARSE_SPLINES; PARITY UNPINNED),
    through the thin C-ABI on device 0; it combines with every switch above but upsampling= (a sequence is opened with it)."""
    if lf_frames or patches:
        if alpha or ycbcr or wide or (patches and not lf_frames and orient):
            return "TODO", None
        try:
            seq = Sequence(data, lf_frames=bool(lf_frames), modular_xyb=bool(modular_xyb), colour=bool(colour), patches=bool(patches), blend=bool(blend), noise=bool(noise), splines=bool(splines))
        except J40Error as e:
            if e.code != "Usq?":
                return e.code, None
            seq = None
        if seq is not None:
            try:
                seq.set_output_format(fmt)
                seq.upload(0)
                err, out = seq.next_to_host()
                if not err and (scale or orient):
                    shown = [k for k in range(seq.num_frames) if seq.frame_info(k)["shown"]]
                    fr = seq.frame(shown[0])
                    code = fr.set_scale(scale) if scale else ""
                    if not code and orient:
                        code = fr.set_orientation(1)
                    if code:
                        return code, None
                    err, out = fr.decode_to_host()
                return err, (None if err else out)
            except J40Error as e:
                return e.code, None
            finally:
                seq.close()
    if alpha or scale or ycbcr or orient or wide or modular_xyb or colour or noise or upsampling or splines:
        try:
            fr = Frame(data, ycbcr=bool(ycbcr), wide=bool(wide), noise=bool(noise), upsampling=bool(upsampling), splines=bool(splines))
        except J40Error as e:
            return e.code, None
        try:
            code = fr.set_alpha(1) if alpha else ""
            if not code and modular_xyb:
                code = fr.set_modular_xyb(1)
            if not code and ycbcr:
                code = fr.set_ycbcr(1)
            if not code and colour:
                code = fr.set_colour(1)
            if not code and scale:
                code = fr.set_scale(scale)
            if not code and orient:
                code = fr.set_orientation(1)
            if code:
                return code, None
            fr.set_output_format(fmt)
            fr.upload(0)
            err, out = fr.decode_to_host()
            if not err:   # bytes behind the frame, as the public API looks for them
                err = err4(lib().j40hip_frame_after_frame_status(fr.h))
            return err, (None if err else out)
        except J40Error as e:
            return e.code, None
        finally:
            fr.close()
    img = from_memory(data)
    img.output_format(J40_RGBA, fmt)
    out = None
    if img.next_frame():
        out = (img.frame_pixels_u16x4 if fmt == J40_U16X4 else img.frame_pixels_u8x4)()[0]
    err = img.error()
    img.free()
    return err, out


def decode_region(data: bytes, x, y, w, h, fmt=J40_U8X4, device=0, orient=False, wide=False, colour=False, noise=False, upsampling=False, splines=False):
    """rectangle (x, y, w, h) of the image through the thin C-ABI: returns (err4, ndarray [h, w, 4] or None), uint8 or uint16 with
    fmt=J40_U16X4 -- the crop of what decode() returns, decoded from the pass groups that cover it (Frame.set_region). The verdict is
    the one over the sections that were decoded, then the public API's look behind the frame.
    orient=True: (x, y, w, h) is a rectangle of the DISPLAYED picture -- the frame in the orientation its stream carries; it is mapped
    to stored coordinates (Frame.orient_rect) and the result is the crop of the oriented whole picture, [h, w, 4].
    wide=True, colour=True, noise=True: as decode()'s (a frame with noise: the crop of the full-size picture).
    upsampling=True: as decode()'s; the rectangle lies in the shown-size picture and is cut from it.
    splines=True: as decode()'s (the crop of the full-size picture)."""
    try:
        fr = Frame(data, wide=bool(wide), noise=bool(noise), upsampling=bool(upsampling), splines=bool(splines))
    except J40Error as e:
        return e.code, None
    try:
        if colour:
            code = fr.set_colour(1)
            if code:
                return code, None
        if orient:
            code, stored = fr.orient_rect((x, y, w, h), to_stored=True)
            if not code:
                code = fr.set_orientation(1)
            if code:
                return code, None
            x, y, w, h = stored
        code = fr.set_region(x, y, w, h)
        if code:
            return code, None
        fr.set_output_format(fmt)
        fr.upload(device)
        err, out = fr.decode_to_host()
        if not err:   # bytes behind the frame, as the public API looks for them
            err = err4(lib().j40hip_frame_after_frame_status(fr.h))
        return err, (None if err else out)
    except J40Error as e:
        return e.code, None
    finally:
        fr.close()


def decode_timed(buf, size, want_pixels=False):
    """the reference's call sequence (dj40.c) on an existing ctypes buffer, timed from j40_from_memory to the return of
    j40_frame_pixels_u8x4 -- the pixels are then in host memory, in the image's own plane; no copy into numpy inside the clock.
    Returns (err4, milliseconds, pixels or None)"""
    import time
    L = lib()
    img = Image()
    t0 = time.perf_counter()
    L.j40_from_memory(C.byref(img._img), buf, size, None)
    img._live = True
    img.output_format()
    ok = img.next_frame()
    px = None
    if ok:
        fr = L.j40_current_frame(C.byref(img._img))
        px = L.j40_frame_pixels_u8x4(C.byref(fr), J40_RGBA)
    ms = (time.perf_counter() - t0) * 1e3
    err = img.error()
    out = None
    if ok and want_pixels and not err:
        rows = np.ctypeslib.as_array(C.cast(px.data, C.POINTER(C.c_uint8)), shape=(px.height, px.stride_bytes))
        out = rows[:, : px.width * 4].reshape(px.height, px.width, 4).copy()
    img.free()
    return err, ms, out


INFO_FIELDS = ["width", "height", "is_modular", "num_lf_groups", "num_groups", "num_passes", "nb_block_ctx", "block_ctx_size",
               "num_hf_presets", "global_scale", "quant_lf", "x_qm_scale", "b_qm_scale", "nb_qf_thr", "nb_lf_thr0", "nb_lf_thr1",
               "nb_lf_thr2", "group_size_shift", "bpp", "num_extra_channels", "xyb_encoded"]


class Restoration(C.Structure):
    """j40hip_restoration (include/j40hip.h): the frame header's RestorationFilter bundle"""
    _fields_ = [("gab_enabled", C.c_int32), ("gab_weights", C.c_float * 6), ("epf_iters", C.c_int32), ("epf_sharp_lut", C.c_float * 8), ("epf_channel_scale", C.c_float * 3),
                ("epf_quant_mul", C.c_float), ("epf_pass0_sigma_scale", C.c_float), ("epf_pass2_sigma_scale", C.c_float), ("epf_border_sad_mul", C.c_float), ("epf_sigma_for_modular", C.c_float)]

    def as_list(self):
        """the 24 numbers in the order oracle/ref_harness.c's ref_stage_restoration writes them"""
        return ([float(self.gab_enabled)] + list(self.gab_weights) + [float(self.epf_iters)] + list(self.epf_sharp_lut) + list(self.epf_channel_scale)
                + [self.epf_quant_mul, self.epf_pass0_sigma_scale, self.epf_pass2_sigma_scale, self.epf_border_sad_mul, self.epf_sigma_for_modular])

    def params15(self):
        """sharp_lut[8], channel_scale[3], quant_mul, pass0, pass2, border_sad_mul: what the checkers' filter entry points take"""
        return np.array(list(self.epf_sharp_lut) + list(self.epf_channel_scale) + [self.epf_quant_mul, self.epf_pass0_sigma_scale, self.epf_pass2_sigma_scale, self.epf_border_sad_mul], np.float32)


def kat_device_orient(src, orientation, fmt=None, pad=0, device=0):
    """k_orient alone (j40hip_kat_device_orient): src [h, w, 4] uint8 or uint16 -> (err4, [oh, ow, 4] of the same dtype, guard) -- the
    output's rows carry `pad` guard bytes filled with 0xA5 beforehand; guard: they all came back untouched. fmt: the format to ask
    for (default: the array's own)"""
    import torch
    src = np.ascontiguousarray(src)
    h, w = src.shape[:2]
    pb = 4 * src.dtype.itemsize
    if fmt is None:
        fmt = J40_U16X4 if pb == 8 else J40_U8X4
    ow, oh = (h, w) if 5 <= orientation <= 8 else (w, h)
    stride = ow * pb + pad
    dev = "cuda:%d" % device
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1)).to(dev)
    d_out = torch.full((oh * stride,), 0xA5, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(device)
    code = err4(lib().j40hip_kat_device_orient(d_out.data_ptr(), stride, d_src.data_ptr(), w * pb, w, h, int(orientation), int(fmt), stream.cuda_stream))
    stream.synchronize()
    if code:
        return code, None, True
    host = d_out.cpu().numpy().reshape(oh, stride)
    guard = bool((host[:, ow * pb:] == 0xA5).all())
    return "", np.ascontiguousarray(host[:, :ow * pb]).view(src.dtype).reshape(oh, ow, 4), guard


def colour_gamut_matrix(enc_words):
    """j40hip_colour_gamut_matrix (host only): (err4, P [3, 3] float64: linear sRGB / D65 -> the encoding's primaries and white point,
    lum [3]: the luminance of the three target-space values) for an encoding given as Frame.colour_encoding(words=True) states it"""
    import numpy as np
    enc = np.ascontiguousarray(enc_words, np.int32)
    p = np.zeros(9, np.float64); lum = np.zeros(3, np.float64)
    code = err4(lib().j40hip_colour_gamut_matrix(enc.ctypes.data, p.ctypes.data, lum.ctypes.data))
    return code, p.reshape(3, 3), lum


COLOUR_TABLE_FLOATS = 258 + 48 * 128 // 4


def colour_table(enc_words, intensity_target):
    """j40hip_colour_table (host only): (err4, table float32 [COLOUR_TABLE_FLOATS], (first bucket, last bucket)) -- the threshold table an
    8-bit frame's colour tail uses for the encoding's curve; "Ucs?": the curve has none"""
    import numpy as np
    enc = np.ascontiguousarray(enc_words, np.int32)
    table = np.zeros(COLOUR_TABLE_FLOATS, np.float32); rng = np.zeros(2, np.int32)
    code = err4(lib().j40hip_colour_table(enc.ctypes.data, float(intensity_target), table.ctypes.data, table.size, rng.ctypes.data))
    return code, table, (int(rng[0]), int(rng[1]))


def kat_device_colour_tail(xyb, colour_consts, enc_words, lum, bpp, fmt=J40_U8X4, use_table=True, pad=0, device=0):
    """k_colour_tail alone (j40hip_kat_device_colour_tail): xyb [3, h, w] float32 (X, Y, B), colour_consts the 15 floats of
    Frame.colour_consts() with the matrix the tail is to use in [0:9], the encoding's 16 words, lum [3]. An 8-bit frame takes the curve's
    threshold table (colour_table) where it has one, unless use_table=False. Returns (err4, pixels [h, w, 4] uint8 or uint16). Rows
    `pad` pixels longer than the image; the padding must come back untouched (asserted here)"""
    import numpy as np
    import torch
    xyb = np.ascontiguousarray(xyb, np.float32)
    _, h, w = xyb.shape
    pb = 8 if fmt == J40_U16X4 else 4
    dev = torch.device("cuda", device)
    cc = np.ascontiguousarray(colour_consts, np.float32); enc = np.ascontiguousarray(enc_words, np.int32); lm = np.ascontiguousarray(lum, np.float32)
    table, rng = None, np.zeros(2, np.int32)
    if bpp == 8 and use_table:
        code, t, r = colour_table(enc, cc[12])
        if not code:
            table, rng = t, np.array(r, np.int32)
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(xyb).to(dev)
        d_table = torch.from_numpy(table).to(dev) if table is not None else None
        out = torch.full((h, (w + pad) * pb), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        code = err4(lib().j40hip_kat_device_colour_tail(d_in.data_ptr(), w, h, cc.ctypes.data, enc.ctypes.data, lm.ctypes.data, int(bpp),
                                                         d_table.data_ptr() if d_table is not None else None, rng.ctypes.data, fmt, out.data_ptr(), (w + pad) * pb, None))
        torch.cuda.synchronize(dev)
        host = out.cpu().numpy()
    if code:
        return code, None
    assert (host[:, w * pb:] == 0xA5).all(), "k_colour_tail wrote behind a row's pixels"
    px = np.ascontiguousarray(host[:, :w * pb])
    return "", (px.view(np.uint16) if pb == 8 else px).reshape(h, w, 4)


def kat_device_modular_xyb(planes, alpha, m, colour_consts, bpp, fmt=J40_U8X4, pad=0, device=0):
    """the Modular XYB kernels alone (j40hip_kat_device_modular_xyb): planes [3, h, w] int16 or int32 (c0, c1, c2), alpha [h, w] of the
    same dtype or None, m [3], colour_consts [15] -> (err4, fused [h, w, 4], two_kernel [h, w, 4], xyb [3, h, w] float32, guard):
    k_modular_xyb_pack's pixels; those of k_modular_to_xyb followed by the VarDCT colour tail's kernel; the planes in between. Rows
    carry `pad` guard bytes filled with 0xA5 beforehand; guard: they all came back untouched."""
    import torch
    planes = np.ascontiguousarray(planes)
    assert planes.dtype in (np.int16, np.int32) and planes.ndim == 3 and planes.shape[0] == 3
    _, h, w = planes.shape
    pb = 8 if fmt == J40_U16X4 else 4
    stride = w * pb + pad
    dev = "cuda:%d" % device
    d_planes = [torch.from_numpy(planes[c].copy()).to(dev) for c in range(3)]
    d_alpha = None if alpha is None else torch.from_numpy(np.ascontiguousarray(alpha, planes.dtype)).to(dev)
    d_fused = torch.full((h * stride,), 0xA5, dtype=torch.uint8, device=dev)
    d_two = torch.full((h * stride,), 0xA5, dtype=torch.uint8, device=dev)
    d_xyb = torch.zeros((3, h, w), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * 3)(*[p.data_ptr() for p in d_planes])
    mm = np.ascontiguousarray(m, np.float32); cc = np.ascontiguousarray(colour_consts, np.float32)
    assert mm.size == 3 and cc.size == 15
    stream = torch.cuda.current_stream(device)
    code = err4(lib().j40hip_kat_device_modular_xyb(ptrs, d_alpha.data_ptr() if d_alpha is not None else None, planes.dtype.itemsize, w, h, mm.ctypes.data, cc.ctypes.data,
                                                    int(bpp), int(fmt), d_fused.data_ptr(), d_two.data_ptr(), stride, d_xyb.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    if code:
        return code, None, None, None, True
    dt = np.uint16 if pb == 8 else np.uint8
    hosts = [t.cpu().numpy().reshape(h, stride) for t in (d_fused, d_two)]
    guard = all(bool((x[:, w * pb:] == 0xA5).all()) for x in hosts)
    fused, two = [np.ascontiguousarray(x[:, :w * pb]).view(dt).reshape(h, w, 4) for x in hosts]
    return "", fused, two, d_xyb.cpu().numpy(), guard


def kat_device_xyb_to_rgba(xyb, colour_consts, bpp, fmt=J40_U8X4, device=0):
    """the VarDCT colour tail's kernel alone (k_xyb_to_rgba through j40hip_kat_device_modular_xyb_launch, kernel 2): xyb [3, h, w] float32
    (X, Y, B), colour_consts the 15 floats of Frame.colour_consts() -> (err4, pixels [h, w, 4] uint8 or uint16), A opaque"""
    import torch
    xyb = np.ascontiguousarray(xyb, np.float32)
    _, h, w = xyb.shape
    pb = 8 if fmt == J40_U16X4 else 4
    dev = "cuda:%d" % device
    cc = np.ascontiguousarray(colour_consts, np.float32); mm = np.zeros(3, np.float32)
    assert cc.size == 15
    size = int(lib().j40hip_kat_device_colour_frame(cc.ctypes.data, int(bpp), None, 0))
    d_frame = torch.zeros(size, dtype=torch.uint8, device=dev)
    d_in = torch.from_numpy(xyb).to(dev)
    d_out = torch.zeros((h, w * pb), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    if lib().j40hip_kat_device_colour_frame(cc.ctypes.data, int(bpp), d_frame.data_ptr(), size) != size:
        return "!gpu", None
    ptrs = (C.c_void_p * 3)(*[d_in[c].data_ptr() for c in range(3)])
    with torch.cuda.device(dev):
        code = err4(lib().j40hip_kat_device_modular_xyb_launch(2, ptrs, 4, w, h, mm.ctypes.data, cc.ctypes.data, int(bpp), int(fmt), d_out.data_ptr(), w * pb, d_frame.data_ptr(), None))
        torch.cuda.synchronize(dev)
    if code:
        return code, None
    px = d_out.cpu().numpy()
    return "", (px.view(np.uint16) if pb == 8 else px).reshape(h, w, 4)


def kat_device_patches(planes, slots, placements, device=0):
    """k_patch_blend alone (j40hip_kat_device_patches): planes [3, h, w] float32 (X, Y, B); slots: four entries, each None or [3, sh, sw]
    float32; placements: rows of nine integers x, y, w, h, x0, y0, slot, mode, clamp in dictionary order -> (err4, the planes after the
    patches or None, the workgroups launched). The planes sit between guard floats, which must come back untouched (asserted here)"""
    import torch
    planes = np.ascontiguousarray(planes, np.float32)
    _, h, w = planes.shape
    dev = "cuda:%d" % device
    guard = 64
    buf = np.full(guard + planes.size + guard, 12345.0, np.float32)
    buf[guard:guard + planes.size] = planes.ravel()
    d_buf = torch.from_numpy(buf).to(dev)
    d_slots = [None if s is None else torch.from_numpy(np.ascontiguousarray(s, np.float32)).to(dev) for s in slots]
    ptrs = (C.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in d_slots])
    sw = np.array([0 if s is None else s.shape[2] for s in slots], np.int32); sh = np.array([0 if s is None else s.shape[1] for s in slots], np.int32)
    pl = np.ascontiguousarray(placements, np.int32).reshape(-1, 9)
    tiles = C.c_int32(0)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        code = err4(lib().j40hip_kat_device_patches(d_buf.data_ptr() + 4 * guard, w, h, ptrs, sw.ctypes.data, sh.ctypes.data, pl.ctypes.data, len(pl), C.byref(tiles), None))
        torch.cuda.synchronize(dev)
    host = d_buf.cpu().numpy()
    assert (host[:guard] == 12345.0).all() and (host[-guard:] == 12345.0).all(), "k_patch_blend wrote outside the planes"
    if code:
        return code, None, 0
    return "", host[guard:guard + planes.size].reshape(3, h, w).copy(), int(tiles.value)


def set_upsampling_defaults(k, weights):
    """the standard's default upsampling weights for k = 2, 4 or 8 (15, 55 or 210 numbers: the upper triangle of the symmetric matrix,
    row by row), supplied once by the application -- nothing in this package holds them; process-wide. Frames parsed afterwards that
    carry no custom table for their K copy them; until then, and after weights=None, such frames answer "updf". Returns the err4 ("rnge": another k or count)"""
    if weights is None:      # (takes the table back: frames parsed afterwards answer "updf" again)
        return err4(lib().j40hip_set_upsampling_defaults(int(k), None, 0))
    w = np.ascontiguousarray(weights, np.float32).ravel()
    if w.size == 0:
        return "rnge"
    return err4(lib().j40hip_set_upsampling_defaults(int(k), w.ctypes.data, int(w.size)))


def kat_upsampling_kernel(k, weights):
    """j40hip_kat_upsampling_kernel: the expanded table [k, k, 5, 5] of the packed weights -- [oy, ox, sy, sx]: what output phase (ox, oy)
    gives the coded sample at (sx - 2, sy - 2); (err4, ndarray or None)"""
    w = np.ascontiguousarray(weights, np.float32).ravel()
    if k not in (2, 4, 8) or w.size != {2: 15, 4: 55, 8: 210}[k]:
        return "rnge", None
    out = np.zeros((k, k, 5, 5), np.float32)
    code = err4(lib().j40hip_kat_upsampling_kernel(int(k), w.ctypes.data, out.ctypes.data))
    return code, (None if code else out)


def kat_host_upsample(planes, k, weights, out_w=None, out_h=None, tiled=False):
    """k_upsample's host twin (j40hip_kat_host_upsample): planes [3, h, w] float32 -> (err4, [3, out_h, out_w] or None); tiled: the
    kernel's tile functions thread by thread instead of the rule sample by sample"""
    planes = np.ascontiguousarray(planes, np.float32)
    _, h, w = planes.shape
    out_w = k * w if out_w is None else out_w; out_h = k * h if out_h is None else out_h
    wt = np.ascontiguousarray(weights, np.float32).ravel()
    if k not in (2, 4, 8) or wt.size != {2: 15, 4: 55, 8: 210}[k] or out_w <= 0 or out_h <= 0:
        return "rnge", None
    out = np.zeros((3, out_h, out_w), np.float32)
    code = err4(lib().j40hip_kat_host_upsample(planes.ctypes.data, w, h, int(k), wt.ctypes.data, int(out_w), int(out_h), out.ctypes.data, 1 if tiled else 0))
    return code, (None if code else out)


def kat_device_upsample(planes, k, weights, out_w=None, out_h=None, device=0, want_ms=False):
    """k_upsample alone (j40hip_kat_device_upsample): planes [3, h, w] float32 -> (err4, [3, out_h, out_w] or None); with want_ms a third
    entry, the kernel's device time in ms. The output sits between guard floats, which must come back untouched (asserted here)"""
    import torch
    planes = np.ascontiguousarray(planes, np.float32)
    _, h, w = planes.shape
    out_w = k * w if out_w is None else out_w; out_h = k * h if out_h is None else out_h
    wt = np.ascontiguousarray(weights, np.float32).ravel()
    if k not in (2, 4, 8) or wt.size != {2: 15, 4: 55, 8: 210}[k] or out_w <= 0 or out_h <= 0:
        return ("rnge", None) + ((None,) if want_ms else ())
    dev = "cuda:%d" % device
    guard = 64
    n = 3 * out_h * out_w
    d_in = torch.from_numpy(planes).to(dev)
    d_out = torch.full((guard + n + guard,), 12345.0, dtype=torch.float32, device=dev)
    ms = C.c_float(0.0)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        code = err4(lib().j40hip_kat_device_upsample(d_in.data_ptr(), w, h, int(k), wt.ctypes.data, int(out_w), int(out_h), d_out.data_ptr() + 4 * guard, None, C.byref(ms) if want_ms else None))
        torch.cuda.synchronize(dev)
    host = d_out.cpu().numpy()
    assert (host[:guard] == 12345.0).all() and (host[-guard:] == 12345.0).all(), "k_upsample wrote outside the planes"
    if code:
        return (code, None) + ((None,) if want_ms else ())
    return ("", host[guard:guard + n].reshape(3, out_h, out_w).copy()) + ((float(ms.value),) if want_ms else ())


def kat_device_splines(planes, segments, device=0, want_ms=False):
    """k_spline_draw alone (j40hip_kat_device_splines): planes [3, h, w] float32 (X, Y, B), segments [n, 12] uint32 words as
    Frame.spline_segments() gives them -> (err4, the planes after the splines or None, the tiles launched); with want_ms a fourth
    entry, the kernel's device time in ms. The planes sit between guard floats, which must come back untouched (asserted here)"""
    import torch
    planes = np.ascontiguousarray(planes, np.float32)
    _, h, w = planes.shape
    segments = np.ascontiguousarray(segments, np.uint32).reshape(-1, 12)
    dev = "cuda:%d" % device
    guard = 64
    buf = np.full(guard + planes.size + guard, 12345.0, np.float32)
    buf[guard:guard + planes.size] = planes.ravel()
    d_buf = torch.from_numpy(buf).to(dev)
    tiles = C.c_int64(0)
    ms = C.c_float(0.0)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        code = err4(lib().j40hip_kat_device_splines(d_buf.data_ptr() + 4 * guard, w, h, segments.ctypes.data, segments.shape[0], C.byref(tiles), None, C.byref(ms) if want_ms else None))
        torch.cuda.synchronize(dev)
    host = d_buf.cpu().numpy()
    assert (host[:guard] == 12345.0).all() and (host[-guard:] == 12345.0).all(), "k_spline_draw wrote outside the planes"
    if code:
        return (code, None, 0) + ((None,) if want_ms else ())
    out = ("", host[guard:guard + planes.size].reshape(3, h, w).copy(), int(tiles.value))
    return out + ((float(ms.value),) if want_ms else ())


def kat_device_noise(planes, group_dim, lut, ytox, ytob, visible=0, nonvisible=0, device=0, want_ms=False):
    """k_noise_fill and k_noise_add alone (j40hip_kat_device_noise): planes [3, h, w] float32 (X, Y, B) -> (err4, the planes after the noise
    or None, the raw planes [3, h, w] the fill made -- zeros for a LUT of zeros, which launches nothing); with want_ms a fourth entry, the
    two kernels' device time in ms. The planes sit between guard floats, which must come back untouched (asserted here)"""
    import torch
    planes = np.ascontiguousarray(planes, np.float32)
    _, h, w = planes.shape
    dev = "cuda:%d" % device
    guard = 64
    buf = np.full(guard + planes.size + guard, 12345.0, np.float32)
    buf[guard:guard + planes.size] = planes.ravel()
    d_buf = torch.from_numpy(buf).to(dev)
    d_raw = torch.zeros(guard + planes.size + guard, dtype=torch.float32, device=dev)
    lut = np.ascontiguousarray(lut, np.float32)
    assert lut.size == 8
    ms = np.zeros(2, np.float32)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        code = err4(lib().j40hip_kat_device_noise(d_buf.data_ptr() + 4 * guard, w, h, int(group_dim), lut.ctypes.data, float(ytox), float(ytob), int(visible), int(nonvisible),
                                                  d_raw.data_ptr() + 4 * guard, None, ms.ctypes.data if want_ms else None))
        torch.cuda.synchronize(dev)
    host = d_buf.cpu().numpy(); raw = d_raw.cpu().numpy()
    assert (host[:guard] == 12345.0).all() and (host[-guard:] == 12345.0).all(), "k_noise_add wrote outside the planes"
    assert (raw[:guard] == 0.0).all() and (raw[-guard:] == 0.0).all(), "the raw planes' copy wrote outside them"
    if code:
        return (code, None, None) + ((None,) if want_ms else ())
    out = ("", host[guard:guard + planes.size].reshape(3, h, w).copy(), raw[guard:guard + planes.size].reshape(3, h, w).copy())
    return out + (((float(ms[0]), float(ms[1])),) if want_ms else ())


def kat_device_srgb_u16(values, bpp):
    """j40hip_kat_device_srgb_u16: linear values -> the 16-bit output sample at bit depth bpp, on the device; returns (err4, uint16 array)"""
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(v.size, np.uint16)
    code = lib().j40hip_kat_device_srgb_u16(v.ctypes.data, v.size, int(bpp), out.ctypes.data)
    return err4(code), out


def kat_device_restoration(planes, sharpness, hfmul_inv, r, mode=1, device=0):
    """j40hip_kat_device_restoration: the filter kernels on caller planes [3, h, w] float32 (a copy is filtered and returned with the
    reciprocal-sigma plane); returns (4-char code, planes, sigma)"""
    a = np.ascontiguousarray(planes, np.float32).copy()
    _, h, w = a.shape
    sh = np.ascontiguousarray(sharpness, np.int16); hf = np.ascontiguousarray(hfmul_inv, np.float32)
    sigma = np.zeros(((h + 7) // 8, (w + 7) // 8), np.float32)
    code = lib().j40hip_kat_device_restoration(a.ctypes.data, w, h, sh.ctypes.data, hf.ctypes.data, C.byref(r), mode, device, sigma.ctypes.data)
    return err4(code), a, sigma


class Frame:
    """thin C-ABI (include/j40hip.h): host parse, plan upload, hot path on a HIP stream"""

    def __init__(self, data: bytes, threads: int = 4, lf_device=None, lf_only=False, ycbcr=False, wide=False, noise=False, upsampling=False, splines=False):
        """lf_device: a HIP device index -- the LfGroup streams are decoded there instead of on the host (j40hip_frame_parse_on).
        lf_only: parse what the LF preview needs and nothing more (J40HIP_PARSE_LF_ONLY): `data` may end at lf_end(); such a frame
        can only be previewed (decode_lf_to_host, decode_lf).
        ycbcr: YCbCr frames are asked for (J40HIP_PARSE_YCBCR): a frame with subsampled channels is parsed instead of refused; serving
        it still takes set_ycbcr(1) (or J40HIP_YCBCR=1)
        wide: wide Modular frames are asked for (J40HIP_PARSE_WIDE): an image with 32-bit Modular buffers is parsed instead of refused
        with "fm32", and its Modular frame is decoded with int32 sample planes (wide())
        noise: photon noise is asked for (J40HIP_PARSE_NOISE; PARITY UNPINNED): a frame with has_noise is parsed instead of refused
        with "TODO" and every decode adds its noise (noise_params(), noise_launches(), read_xyb(4))
        splines: splines are asked for (J40HIP_PARSE_SPLINES; PARITY UNPINNED): a frame with has_splines is parsed instead of refused
        with "TODO" and every decode draws them (splines(), spline_segments(), spline_launches(), read_xyb(6)); "spln": a damaged one
        upsampling: upsampling is asked for (J40HIP_PARSE_UPSAMPLING; PARITY UNPINNED): custom upsampling weights and a frame coded at
        1:2, 1:4 or 1:8 are parsed instead of refused with "TODO"; width and height are the SHOWN size, which every decode writes
        (upsampling(), coded_size(), read_xyb(5))"""
        L = lib()
        self._buf = C.create_string_buffer(data, len(data))
        err = C.c_uint32()
        flags = (PARSE_LF_ONLY if lf_only else 0) | (PARSE_YCBCR if ycbcr else 0) | (PARSE_WIDE if wide else 0) | (PARSE_NOISE if noise else 0) | (PARSE_UPSAMPLING if upsampling else 0) | (PARSE_SPLINES if splines else 0)
        if lf_device is None:
            self.h = L.j40hip_frame_parse_ex(self._buf, len(data), threads, flags, C.byref(err))
        else:
            self.h = L.j40hip_frame_parse_on(self._buf, len(data), threads, 1 | flags, int(lf_device), None, C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_frame_parse")
        info = np.zeros(32, np.int64)
        L.j40hip_frame_info(self.h, info.ctypes.data)
        self.info = dict(zip(INFO_FIELDS, info.tolist()))
        self.width, self.height = self.info["width"], self.info["height"]
        self.codestream_size = L.j40hip_frame_codestream_size(self.h)

    @classmethod
    def parse_streamed(cls, data: bytes, step: int = 4096, threads: int = 4, flags: int = 0, log=None):
        """j40hip_frame_parse_streamed over a buffer that fills up as the parser asks (include/j40hip.h): the buffer starts as
        0xAA bytes and every need(n) reveals the stream's bytes up to n rounded up to a multiple of `step` -- a parser that read a
        byte it had not asked for would see rubbish. log (a list) receives every n asked for."""
        L = lib()
        self = cls.__new__(cls)
        n = len(data)
        self._buf = (C.c_uint8 * max(n, 1)).from_buffer(bytearray(b"\xaa" * max(n, 1)))
        have = [0]
        import threading
        lock = threading.Lock()

        def need(_ctx, upto):
            with lock:
                if log is not None:
                    log.append(int(upto))
                want = min(n, (int(upto) + step - 1) // step * step)
                if want > have[0]:
                    C.memmove(C.addressof(self._buf) + have[0], data[have[0]:want], want - have[0])
                    have[0] = want

        def have_now(_ctx):
            with lock:
                return have[0]

        NEED = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t)
        HAVE = C.CFUNCTYPE(C.c_size_t, C.c_void_p)
        self._cb = (NEED(need), HAVE(have_now))
        L.j40hip_frame_parse_streamed.restype = C.c_void_p
        L.j40hip_frame_parse_streamed.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, NEED, HAVE, C.c_void_p, C.POINTER(C.c_uint32)]
        err = C.c_uint32()
        self.h = L.j40hip_frame_parse_streamed(self._buf, n, threads, flags, self._cb[0], self._cb[1], None, C.byref(err))
        self.revealed = have[0]
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_frame_parse_streamed")
        need(None, n)   # (the rest arrives before anything else looks at the buffer)
        info = np.zeros(32, np.int64)
        L.j40hip_frame_info(self.h, info.ctypes.data)
        self.info = dict(zip(INFO_FIELDS, info.tolist()))
        self.width, self.height = self.info["width"], self.info["height"]
        self.codestream_size = L.j40hip_frame_codestream_size(self.h)
        return self

    @classmethod
    def from_lf_bundle(cls, blob: bytes):
        """a frame handle from the blob Frame.lf_bundle() of another process made (VarDCT frames; nothing is parsed here)"""
        L = lib()
        self = cls.__new__(cls)
        self._buf = C.create_string_buffer(blob, len(blob))
        err = C.c_uint32()
        self.h = L.j40hip_frame_from_lf_bundle(self._buf, len(blob), C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_frame_from_lf_bundle")
        info = np.zeros(32, np.int64)
        L.j40hip_frame_info(self.h, info.ctypes.data)
        self.info = dict(zip(INFO_FIELDS, info.tolist()))
        self.width, self.height = self.info["width"], self.info["height"]
        self.codestream_size = L.j40hip_frame_codestream_size(self.h)
        return self

    def lf_on_device(self):
        return bool(lib().j40hip_frame_lf_on_device(self.h))

    def lf_bundle(self) -> bytes:
        """the parsed frame (codestream + LF bundle + tables) as one relocatable blob: what rank 0 of a sharded decode can
        broadcast instead of the codestream"""
        L = lib()
        err = C.c_uint32()
        need = L.j40hip_frame_lf_bundle(self.h, None, 0, C.byref(err))
        self._chk(err.value, "in j40hip_frame_lf_bundle")
        out = C.create_string_buffer(need)
        if L.j40hip_frame_lf_bundle(self.h, out, need, C.byref(err)) != need:
            self._chk(err.value or int.from_bytes(b"!mem", "big"), "in j40hip_frame_lf_bundle")
        return out.raw

    @classmethod
    def _borrowed(cls, handle, owner):
        """a frame handle somebody else owns (a Sequence's coded frame): every method works, close() leaves the handle alone"""
        self = cls.__new__(cls)
        self.h, self._owner = handle, owner
        info = np.zeros(32, np.int64)
        lib().j40hip_frame_info(self.h, info.ctypes.data)
        self.info = dict(zip(INFO_FIELDS, info.tolist()))
        self.width, self.height = self.info["width"], self.info["height"]
        self.codestream_size = lib().j40hip_frame_codestream_size(self.h)
        return self

    def close(self):
        if self.h and getattr(self, "_owner", None) is None:
            lib().j40hip_frame_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, code, where):
        if code:
            raise J40Error(err4(code), where)

    def upload(self, device=0):
        self._chk(lib().j40hip_frame_upload(self.h, device), "in j40hip_frame_upload")

    def force_dense(self, dense=True):
        """dense coefficient planes instead of event lists for the next upload (what the library does by itself after "evof")"""
        lib().j40hip_frame_force_dense(self.h, 1 if dense else 0)

    def coop_sections(self):
        """(sections the wave-cooperative Modular kernel takes, sections of the plan); (-1, 0) without a Modular plan"""
        total = C.c_int32(0)
        n = lib().j40hip_frame_coop_sections(self.h, C.byref(total))
        return int(n), int(total.value)

    def quad_sections(self):
        return int(lib().j40hip_frame_quad_sections(self.h))

    def split_sections(self):
        """sections the two-pass Modular decoder takes (position-only MA trees; modular_split.hip)"""
        return int(lib().j40hip_frame_split_sections(self.h))

    def section_sizes(self):
        """bytes of every pass-group section (pass-major), from the TOC"""
        n = lib().j40hip_frame_section_sizes(self.h, None)
        a = np.zeros(n, np.int64)
        lib().j40hip_frame_section_sizes(self.h, a.ctypes.data)
        return a

    def set_group_range(self, first, count):
        self._chk(lib().j40hip_frame_set_group_range(self.h, first, count), "in j40hip_frame_set_group_range")

    def decode(self, rgba_ptr, stride_bytes, stream=0):
        self._chk(lib().j40hip_frame_decode(self.h, rgba_ptr, stride_bytes, stream), "in j40hip_frame_decode")

    def decode_timed(self, rgba_ptr, stride_bytes, stream=0):
        ms = np.zeros(3, np.float32)
        self._chk(lib().j40hip_frame_decode_timed(self.h, rgba_ptr, stride_bytes, stream, ms.ctypes.data), "in j40hip_frame_decode_timed")
        return ms

    def status(self):
        return err4(lib().j40hip_frame_status(self.h))

    def set_output_format(self, fmt):
        """J40_U8X4 (default) or J40_U16X4: what the decode entry points write for this frame (j40hip_frame_set_output_format)"""
        self._chk(lib().j40hip_frame_set_output_format(self.h, int(fmt)), "in j40hip_frame_set_output_format")

    def output_format(self):
        return int(lib().j40hip_frame_output_format(self.h))

    def decode_to_host(self):
        """(err4, pixels [h, w, 4]): uint8, or uint16 when the frame is set to J40_U16X4; with a region set (set_region) h and w are
        the rectangle's and only it comes back from the device"""
        u16 = self.output_format() == J40_U16X4
        o = self.orientation()
        w, h = o["width"], o["height"]   # (region, scale and orientation counted; none of them: the frame's own size)
        out = np.zeros((h, w, 4), np.uint16 if u16 else np.uint8)
        code = lib().j40hip_frame_decode_to_host(self.h, out.ctypes.data, w * (8 if u16 else 4))
        return err4(code), out

    # ---- region decode (include/j40hip.h) ----
    def set_region(self, x, y, w, h):
        """the decode entry points write rectangle (x, y, w, h) of the frame, w x h pixels, from the pass groups that cover it
        (j40hip_frame_set_region). Returns "" or the refusal: "rnge" (not inside the frame), "Ulf?" (an LF-only frame), "Urg?" (a
        partial group range is set); (0, 0, 0, 0) and the full frame clear the region"""
        return err4(lib().j40hip_frame_set_region(self.h, int(x), int(y), int(w), int(h)))

    def clear_region(self):
        return self.set_region(0, 0, 0, 0)

    def region(self):
        """j40hip_frame_region: the rectangle x, y, w, h (the whole frame without a region); its cover in groups gx0, gy0, gcols, grows;
        set; and of the last decode with a region: widened (to every group), sections (pass-group sections launched), varblocks (what
        the pixel kernels took; 0 for Modular frames)"""
        a = np.zeros(12, np.int32)
        lib().j40hip_frame_region(self.h, a.ctypes.data)
        return dict(zip(["x", "y", "w", "h", "gx0", "gy0", "gcols", "grows", "set", "widened", "sections", "varblocks"], a.tolist()))

    # ---- reduced-size decode (include/j40hip.h) ----
    def set_scale(self, shift):
        """the decode entry points write the whole frame at 1:2 (shift 1) or 1:4 (shift 2), ceil(width / s) x ceil(height / s) pixels,
        every sample the rounded mean of its cell of the full decode on coded levels (j40hip_frame_set_scale); 0: full size.
        Returns "" or the refusal: "rnge" (a shift outside 0..2), "Ulf?" (an LF-only frame), "Usc?" (a region or a partial group
        range is set, or the handle comes from Sequence.frame)"""
        shift = int(shift)
        if not -2 ** 31 <= shift < 2 ** 31:
            return "rnge"
        return err4(lib().j40hip_frame_set_scale(self.h, shift))

    def scale(self):
        """j40hip_frame_scale: shift; width, height at that shift; and of the last decode at a shift above 0: staged (1: through a
        full-size staging image, 0: the kernels wrote the small image, -1: none yet), staging_bytes"""
        a = np.zeros(5, np.int32)
        lib().j40hip_frame_scale(self.h, a.ctypes.data)
        return dict(zip(["shift", "width", "height", "staged", "staging_bytes"], a.tolist()))

    # ---- oriented output (include/j40hip.h) ----
    def set_orientation(self, mode):
        """1: the decode entry points write the picture in the orientation the stream carries (EXIF numbering 1..8; ow x oh is h x w
        from 5 on), applied last by k_orient to what the handle writes in stored order; 0: stored order; -1 (the default): as
        J40HIP_ORIENT says (j40hip_frame_set_orientation). Returns "" or "Uor?" (mode 1 on a handle from Sequence.frame, or on a frame
        with a partial group range whose stream carries an orientation other than 1)"""
        return err4(lib().j40hip_frame_set_orientation(self.h, int(mode)))

    def orientation(self):
        """j40hip_frame_orientation: orientation (the stream's, 1..8); applied (the next decode applies one other than 1); width, height
        the next decode writes (region and scale counted); and of the last decode: went_through_k_orient, staging_bytes"""
        a = np.zeros(6, np.int32)
        lib().j40hip_frame_orientation(self.h, a.ctypes.data)
        return dict(zip(["orientation", "applied", "width", "height", "went_through_k_orient", "staging_bytes"], a.tolist()))

    def orient_rect(self, rect, to_stored=True):
        """(err4, (x, y, w, h)): rectangle `rect` of the whole frame mapped from displayed to stored coordinates (to_stored) or back
        (j40hip_frame_orient_rect); "rnge" and None if it lies outside the frame"""
        try:
            a = np.array([int(v) for v in rect], np.int64)
        except (TypeError, ValueError):
            return "rnge", None
        if a.shape != (4,) or (a < -2 ** 31).any() or (a >= 2 ** 31).any():
            return "rnge", None
        a = a.astype(np.int32)
        out = np.zeros(4, np.int32)
        code = err4(lib().j40hip_frame_orient_rect(self.h, 1 if to_stored else 0, a.ctypes.data, out.ctypes.data))
        return code, (None if code else tuple(out.tolist()))

    def two_phase_sections(self):
        """how decode_to_host last went: k > 0 = two phases with the k longest sections beside the others, 0 = one, -1 = not yet"""
        return lib().j40hip_frame_two_phase_sections(self.h)

    # ---- restoration filters (include/j40hip.h) ----
    def restoration(self):
        """the frame header's RestorationFilter bundle as parsed (j40hip_restoration)"""
        r = Restoration()
        lib().j40hip_frame_restoration(self.h, C.byref(r))
        return r

    def set_restoration(self, mode):
        """-1: as J40HIP_RESTORATION says, 0: off (what j40 does), 1: the filters the frame signals, 2: exactly as j40's routines stand"""
        lib().j40hip_frame_set_restoration(self.h, int(mode))

    # ---- the alpha channel of VarDCT frames (include/j40hip.h) ----
    def set_alpha(self, mode):
        """-1: as J40HIP_ALPHA says (default), 0: drop (A = 255, the reference's pixels), 1: keep the alpha extra channel. Returns "" or
        the refusal: "TODO" (mode 1 on a frame keep mode does not serve; the frame is left as it was), "Ual?" (no alpha channel, or a
        Modular frame, whose alpha is always rendered)"""
        return err4(lib().j40hip_frame_set_alpha(self.h, int(mode)))

    def alpha(self):
        """{"index": the alpha extra channel or -1, "bpp": its depth, "mode": 1 when the next decode keeps alpha, "written": the last decode did}"""
        a = np.zeros(4, np.int32)
        lib().j40hip_frame_alpha(self.h, a.ctypes.data)
        return dict(zip(["index", "bpp", "mode", "written"], a.tolist()))

    # ---- YCbCr VarDCT frames (include/j40hip.h) ----
    def set_ycbcr(self, mode):
        """-1: as J40HIP_YCBCR says (default), 0: refuse YCbCr frames ("TODO", the reference's answer), 1: serve them. Holds from
        the next upload on; returns "" """
        return err4(lib().j40hip_frame_set_ycbcr(self.h, int(mode)))

    def ycbcr(self):
        """{"ycbcr": the frame is a YCbCr VarDCT frame, "shifts": ((hshift, vshift) of Cb, Y, Cr), "used": the last decode went
        through the YCbCr planes and k_ycbcr_tail}"""
        a = np.zeros(8, np.int32)
        lib().j40hip_frame_ycbcr(self.h, a.ctypes.data)
        return {"ycbcr": int(a[0]), "shifts": tuple((int(a[1 + 2 * c]), int(a[2 + 2 * c])) for c in range(3)), "used": int(a[7])}

    def set_modular_xyb(self, mode):
        """a Modular frame of an XYB image: -1 as J40HIP_MODULAR_XYB says, 0 rendered as R, G, B (the reference's pixels), 1 through the
        XYB colour tail (PARITY UNPINNED); returns "" or "Umx?" (mode 1 on a frame the rule does not apply to: VarDCT, not XYB encoded,
        grey, YCbCr, float samples, fewer than 8 bits)"""
        return err4(lib().j40hip_frame_set_modular_xyb(self.h, int(mode)))

    # ---- the colour mode (include/j40hip.h) ----
    def set_colour(self, mode):
        """1: an XYB image is rendered in the colour space its header signals (white point, primaries, transfer function or gamma) by
        k_colour_tail; 0: as sRGB (the reference's pixels); -1 (the default): as J40HIP_COLOUR says (j40hip_frame_set_colour). An image
        whose encoding is the sRGB default decodes the usual way either way. Returns "" or "Ucs?" (want_icc, transfer function 2, grey,
        a YCbCr frame, a Modular frame without set_modular_xyb(1), a partial group range; the frame is left as it was)"""
        return err4(lib().j40hip_frame_set_colour(self.h, int(mode)))

    def colour(self):
        """{applies, in_force, white_point, primaries, transfer (-1 with a gamma), colour_space, used: the last decode went through
        k_colour_tail, curve_evaluated_at_8_bits: ... and it was an 8-bit frame whose curve has no threshold table (linear, or a gamma
        next to nothing), refusal: what set_colour(1) would answer}"""
        import numpy as np
        a = np.zeros(8, np.int32)
        lib().j40hip_frame_colour(self.h, a.ctypes.data)
        return {"applies": bool(a[0]), "in_force": bool(a[1]), "white_point": int(a[2]), "primaries": int(a[3]), "transfer": int(a[4]), "colour_space": int(a[5]),
                "used": bool(a[6]), "curve_evaluated_at_8_bits": int(a[6]) == 2, "refusal": err4(int(a[7]) & 0xffffffff)}

    def colour_encoding(self, words=False):
        """the image header's ColourEncoding as parsed: {colour_space, white_point, white_xy, primaries, primaries_xy (R, G, B),
        have_gamma, gamma, transfer, intent, want_icc}; xy in units of 1e-6 and gamma of 1e-7, the stream's integers (an enum's xy: the
        values it stands for). words=True: the 16 int32 words as j40hip_frame_colour_encoding writes them"""
        import numpy as np
        a = np.zeros(16, np.int32)
        lib().j40hip_frame_colour_encoding(self.h, a.ctypes.data)
        if words:
            return a
        return {"colour_space": int(a[0]), "white_point": int(a[1]), "white_xy": (int(a[2]), int(a[3])), "primaries": int(a[4]),
                "primaries_xy": tuple((int(a[5 + 2 * c]), int(a[6 + 2 * c])) for c in range(3)), "have_gamma": bool(a[11]), "gamma": int(a[12]),
                "transfer": int(a[13]), "intent": int(a[14]), "want_icc": bool(a[15])}

    def modular_xyb(self):
        """{"applies": the rule applies to the frame, "on": it is in force, "sample_bytes": 2 or 4 (0: a VarDCT frame), "used": the last
        decode went through k_modular_xyb_pack / k_modular_to_xyb}"""
        a = np.zeros(4, np.int32)
        lib().j40hip_frame_modular_xyb(self.h, a.ctypes.data)
        return {"applies": int(a[0]), "on": int(a[1]), "sample_bytes": int(a[2]), "used": int(a[3])}

    def wide(self):
        """{"wide": the image has 32-bit Modular buffers, "bpp": its bit depth, "used": the last decode ran the int32 kernels,
        "sample_bytes": bytes per sample of the uploaded frame's planes (0 before an upload)}"""
        a = np.zeros(4, np.int32)
        lib().j40hip_frame_wide(self.h, a.ctypes.data)
        return {"wide": int(a[0]), "bpp": int(a[1]), "used": int(a[2]), "sample_bytes": int(a[3])}

    def read_plane_i16(self, c, shape):
        """after a decode of a narrow Modular frame: channel c of the frame's planes (after the inverse transforms), int16 [shape]"""
        a = np.zeros(shape, np.int16)
        self._chk(lib().j40hip_frame_read_plane_i16(self.h, int(c), a.ctypes.data), "in j40hip_frame_read_plane_i16")
        return a

    def read_plane_i32(self, c, shape):
        """after a decode of a wide frame: channel c of the frame's planes (after the inverse transforms), int32 [shape]"""
        a = np.zeros(shape, np.int32)
        self._chk(lib().j40hip_frame_read_plane_i32(self.h, int(c), a.ctypes.data), "in j40hip_frame_read_plane_i32")
        return a

    def ycbcr_plane_shape(self, c):
        """(rows, columns) of plane c as j40hip_frame_read_ycbcr returns it: the frame's size, or for a subsampled frame the block
        grid padded to whole MCUs at the channel's resolution"""
        sh = self.ycbcr()["shifts"]
        if not any(v for p in sh for v in p):
            return self.height, self.width
        mh, mv = max(p[0] for p in sh), max(p[1] for p in sh)
        fw = -(-self.width // (8 << mh)) << (mh + 3)
        fh = -(-self.height // (8 << mv)) << (mv + 3)
        return fh >> sh[c][1], fw >> sh[c][0]

    def read_ycbcr(self, c):
        """after a decode through the YCbCr path: plane c (0 Cb, 1 Y, 2 Cr) as k_ycbcr_tail read it, float32 [rows, columns]"""
        a = np.zeros(self.ycbcr_plane_shape(c), np.float32)
        self._chk(lib().j40hip_frame_read_ycbcr(self.h, int(c), a.ctypes.data), "in j40hip_frame_read_ycbcr")
        return a

    def sharpness(self, gg):
        gi = self.lf_group_info(gg)
        a = np.zeros((gi["height8"], gi["width8"]), np.int16)
        assert lib().j40hip_frame_sharpness(self.h, gg, a.ctypes.data) == 0
        return a

    def read_xyb(self, stage):
        """after a decode that ran the filters: stage 0 / 1 -> [3, height, width] float32 (before / after them), 2 -> the reciprocal sigmas [h8, w8].
        A Modular frame of an XYB image decoded with set_modular_xyb(1) in force: stage 0 -> the planes X, Y, B by k_modular_to_xyb.
        A frame with patches (Sequence's patches=): stage 3 -> [3, height, width], the planes after k_patch_blend, as the tail read them.
        A frame with noise (noise=True): stage 4 -> the planes after k_noise_add, as the tail read them (with both, stage 3 is "rnge").
        A frame with splines (splines=True): stage 6 -> the planes after k_spline_draw, as the tail read them ("rnge" where noise
        follows: stage 4 then has the planes after both); with patches as well, stage 3 -> the planes between k_patch_blend and k_spline_draw.
        An upsampled frame (upsampling=True): stage 5 -> [3, height, width] of the shown size, the planes k_upsample wrote and the tail
        read; every other stage has the coded size (coded_size())"""
        cw, ch = (self.width, self.height) if stage == 5 else self.coded_size()
        a = np.zeros((3, ch, cw), np.float32) if stage != 2 else np.zeros(((ch + 7) // 8, (cw + 7) // 8), np.float32)
        self._chk(lib().j40hip_frame_read_xyb(self.h, stage, a.ctypes.data), "in j40hip_frame_read_xyb")
        return a

    def upsampling(self):
        """(K, weights): the frame's upsampling (1, 2, 4 or 8) and the table it copied at parse -- the stream's custom one for its K, else
        the defaults set_upsampling_defaults supplied --, float32 [15 / 55 / 210]; empty for K = 1"""
        k = C.c_int32(); n = C.c_int32(); w = np.zeros(210, np.float32)
        self._chk(lib().j40hip_frame_upsampling(self.h, C.byref(k), w.ctypes.data, C.byref(n)), "in j40hip_frame_upsampling")
        return int(k.value), w[:int(n.value)].copy()

    def coded_size(self):
        """(width, height) the frame is coded at: ceil(shown / K) for an upsampled frame, else width and height themselves"""
        w = C.c_int32(); h = C.c_int32()
        lib().j40hip_frame_coded_size(self.h, C.byref(w), C.byref(h))
        return int(w.value), int(h.value)

    def upsample_ms(self):
        """with J40HIP_UPSAMPLE_TIMING=1: the device time of k_upsample in the last decode"""
        return float(lib().j40hip_frame_upsample_ms(self.h))

    def splines(self):
        """the splines as parsed (j40hip_frame_splines, j40hip_frame_spline): None for a frame without has_splines, else a dict --
        "quant_adjust", and "splines": a list of dicts with "start" (x, y), "deltas" (the double deltas of the further control points,
        [n, 2] int64) and "coef" ([4, 32] int32: X, Y, B, sigma)"""
        n = C.c_int32(); qa = C.c_int32()
        if not lib().j40hip_frame_splines(self.h, C.byref(n), C.byref(qa)):
            return None
        out = []
        for i in range(n.value):
            start = np.zeros(2, np.int64); npts = C.c_int32(); coef = np.zeros((4, 32), np.int32)
            self._chk(lib().j40hip_frame_spline(self.h, i, start.ctypes.data, C.byref(npts), None, 0, coef.ctypes.data), "in j40hip_frame_spline")
            dd = np.zeros((npts.value, 2), np.int64)
            self._chk(lib().j40hip_frame_spline(self.h, i, None, None, dd.ctypes.data, dd.size, None), "in j40hip_frame_spline")
            out.append({"start": (int(start[0]), int(start[1])), "deltas": dd, "coef": coef})
        return {"quant_adjust": int(qa.value), "splines": out}

    def spline_segments(self):
        """the segments the next decode draws (j40hip_frame_spline_segments): [n, 12] uint32 words -- x0, x1, y0, y1 (int32), cx, cy,
        1 / sigma, sigma * multiplier / 4, colour X, Y, B (float32 bits), a pad -- in drawing order"""
        n = int(lib().j40hip_frame_spline_segments(self.h, None, 0))
        a = np.zeros((n, 12), np.uint32)
        if n:
            lib().j40hip_frame_spline_segments(self.h, a.ctypes.data, n)
        return a

    def spline_bins(self):
        """(the 64 x 32 tiles the segments touch, the (tile, segment) pairs)"""
        a = np.zeros(2, np.int64)
        lib().j40hip_frame_spline_bins(self.h, a.ctypes.data)
        return int(a[0]), int(a[1])

    def spline_launches(self):
        """how often decodes of this handle have launched k_spline_draw (never for a frame whose segments all dropped)"""
        return int(lib().j40hip_frame_spline_launches(self.h))

    def spline_ms(self):
        """with J40HIP_SPLINE_TIMING=1: the device time of k_spline_draw in the last decode"""
        return float(lib().j40hip_frame_spline_ms(self.h))

    def noise_params(self):
        """photon noise (j40hip_frame_noise): None for a frame without has_noise, else a dict -- "lut": the eight NoiseParameters / 1024
        (float32), "seeds": the seed counters (visible, nonvisible) the next decode uses (a sequence's index counts them)"""
        lut = np.zeros(8, np.float32); seeds = np.zeros(2, np.uint32)
        if not lib().j40hip_frame_noise(self.h, lut.ctypes.data, seeds.ctypes.data):
            return None
        return {"lut": lut, "seeds": (int(seeds[0]), int(seeds[1]))}

    def noise_launches(self):
        """how often decodes of this handle have launched k_noise_fill and k_noise_add (never for a LUT of eight zeros)"""
        return int(lib().j40hip_frame_noise_launches(self.h))

    def noise_ms(self):
        """with J40HIP_NOISE_TIMING=1: the device time of (k_noise_fill, k_noise_add) in the last decode"""
        ms = np.zeros(2, np.float32)
        lib().j40hip_frame_noise_ms(self.h, ms.ctypes.data)
        return float(ms[0]), float(ms[1])

    def restoration_ms(self):
        return float(lib().j40hip_frame_restoration_ms(self.h))

    # ---- stage accessors ----
    def lf_group_info(self, gg):
        a = np.zeros(9, np.int32)
        lib().j40hip_frame_lf_group_info(self.h, gg, a.ctypes.data)
        return dict(zip(["left", "top", "width", "height", "width8", "height8", "width64", "height64", "nb_varblocks"], a.tolist()))

    def plane(self, gg, which):
        gi = self.lf_group_info(gg)
        shape, dt = {0: ((gi["height8"], gi["width8"]), np.int32), 1: ((gi["height8"], gi["width8"]), np.uint8),
                     2: ((gi["height64"], gi["width64"]), np.int16), 3: ((gi["height64"], gi["width64"]), np.int16)}[which]
        a = np.zeros(shape, dt)
        assert lib().j40hip_frame_lf_group_plane(self.h, gg, which, a.ctypes.data) == 0
        return a

    def varblocks(self, gg):
        n = self.lf_group_info(gg)["nb_varblocks"]
        a, b = np.zeros(n, np.int32), np.zeros(n, np.float32)
        lib().j40hip_frame_varblocks(self.h, gg, a.ctypes.data, b.ctypes.data)
        return a, b

    def llf(self, gg, c):
        gi = self.lf_group_info(gg)
        a = np.zeros(gi["height8"] * gi["width8"], np.float32)
        lib().j40hip_frame_llf(self.h, gg, c, a.ctypes.data)
        return a

    def dq_matrix(self, idx):
        a = np.zeros((65536, 3), np.float32)
        n = lib().j40hip_frame_dq_matrix(self.h, idx, a.ctypes.data)
        return a[:n].copy()

    def order(self, p, idx, c):
        a = np.zeros(65536, np.int32)
        n = lib().j40hip_frame_order(self.h, p, idx, c, a.ctypes.data)
        return a[:n].copy()

    def block_ctx_map(self):
        a = np.zeros(4096, np.uint8)
        n = lib().j40hip_frame_block_ctx_map(self.h, a.ctypes.data)
        return a[:n].copy()

    def global_plane(self, c):
        w, h = C.c_int32(), C.c_int32()
        if lib().j40hip_frame_global_plane(self.h, c, None, C.byref(w), C.byref(h)) != 0:
            return None
        a = np.zeros((h.value, w.value), np.int16)
        lib().j40hip_frame_global_plane(self.h, c, a.ctypes.data, C.byref(w), C.byref(h))
        return a

    def read_coeffs(self, gg, c):
        gi = self.lf_group_info(gg)
        a = np.zeros(gi["height8"] * gi["width8"] * 64, np.float32)
        self._chk(lib().j40hip_frame_read_coeffs(self.h, gg, c, a.ctypes.data), "in j40hip_frame_read_coeffs")
        return a

    # ---- the LF preview (include/j40hip.h; INTEGRATION.md, "LF preview") ----
    def lf_end(self):
        """bytes of the codestream the preview needs: headers, TOC, LfGlobal and every LfGroup section (single section: all of it)"""
        return int(lib().j40hip_frame_lf_end(self.h))

    def lf_size(self):
        """(w8, h8) = (ceil(width / 8), ceil(height / 8))"""
        w, h = C.c_int32(), C.c_int32()
        lib().j40hip_frame_lf_size(self.h, C.byref(w), C.byref(h))
        return w.value, h.value

    def lf_plane(self, c):
        """channel c (0 X, 1 Y, 2 B) of the dequantised, smoothed LF image, from the host parse: float32 [h8, w8]"""
        w8, h8 = self.lf_size()
        a = np.zeros((h8, w8), np.float32)
        self._chk(lib().j40hip_frame_lf_plane(self.h, int(c), a.ctypes.data), "in j40hip_frame_lf_plane")
        return a

    def read_lf(self, c):
        """the same plane as the device's preview kernel computes it (uploaded frames): float32 [h8, w8]"""
        w8, h8 = self.lf_size()
        a = np.zeros((h8, w8), np.float32)
        self._chk(lib().j40hip_frame_read_lf(self.h, int(c), a.ctypes.data), "in j40hip_frame_read_lf")
        return a

    def colour_consts(self):
        """(opsin_inv_mat [3, 3], opsin_bias [3], intensity_target, kx_lf, kb_lf) as parsed, float32"""
        a = np.zeros(15, np.float32)
        lib().j40hip_frame_colour_consts(self.h, a.ctypes.data)
        return a[:9].reshape(3, 3).copy(), a[9:12].copy(), np.float32(a[12]), np.float32(a[13]), np.float32(a[14])

    def lf_dequant(self):
        """LfGlobal's LF dequantisation m_lf_scaled (X, Y, B) as parsed, float32 [3]"""
        a = np.zeros(3, np.float32)
        lib().j40hip_frame_lf_dequant(self.h, a.ctypes.data)
        return a

    def decode_lf(self, rgba_ptr, stride_bytes, stream=0):
        """the preview into device memory, asynchronously on `stream`"""
        self._chk(lib().j40hip_frame_decode_lf(self.h, rgba_ptr, stride_bytes, stream), "in j40hip_frame_decode_lf")

    def decode_lf_to_host(self):
        """the preview [h8, w8, 4]: uint8, or uint16 when the frame is set to J40_U16X4 (raises J40Error on failure); [w8, h8, 4] where
        an orientation from 5 on is in force (set_orientation)"""
        w8, h8 = self.lf_size()
        o = self.orientation()
        if o["applied"] and o["orientation"] >= 5:
            w8, h8 = h8, w8
        u16 = self.output_format() == J40_U16X4
        out = np.zeros((h8, w8, 4), np.uint16 if u16 else np.uint8)
        self._chk(lib().j40hip_frame_decode_lf_to_host(self.h, out.ctypes.data, w8 * (8 if u16 else 4)), "in j40hip_frame_decode_lf_to_host")
        return out


def frames_decode_lf(frames, rgba_ptrs, strides, stream=0):
    """j40hip_frames_decode_lf: the previews of uploaded frames (LF-only or full) in one launch; returns the 4-char code ("" = launched)"""
    n = len(frames)
    hs = (C.c_void_p * n)(*[f.h for f in frames])
    ptrs = (C.c_void_p * n)(*rgba_ptrs)
    st = (C.c_size_t * n)(*strides)
    return err4(lib().j40hip_frames_decode_lf(hs, n, ptrs, st, stream))


def decode_lf(data: bytes, fmt=J40_U8X4, device=0):
    """the LF preview of one stream (LF-only parse, upload, decode): (err4, [h8, w8, 4] uint8 or uint16 with fmt=J40_U16X4, or None)"""
    err, out = decode_lf_many([data], fmt, device)
    return err, out[0]


def decode_lf_many(datas, fmt=J40_U8X4, device=0):
    """the LF previews of many streams through ONE preview launch (j40hip_frames_decode_lf) into one device buffer: (err4, list of
    arrays). The first stream that fails to parse or upload ends it: its code and no arrays."""
    import torch
    frames = []
    try:
        for d in datas:
            fr = Frame(d, lf_only=True)
            frames.append(fr)
            fr.set_output_format(fmt)
            fr.upload(device)
        px = 8 if fmt == J40_U16X4 else 4
        sizes = [f.lf_size() for f in frames]
        offs = np.cumsum([0] + [w * h * px for w, h in sizes])
        buf = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda:%d" % device)
        stream = torch.cuda.current_stream(device)
        err = frames_decode_lf(frames, [buf.data_ptr() + int(o) for o in offs[:-1]], [w * px for w, _ in sizes], stream.cuda_stream)
        if err:
            return err, [None] * len(datas)
        stream.synchronize()
        host = buf.cpu().numpy()
        dt = np.uint16 if fmt == J40_U16X4 else np.uint8
        return "", [host[offs[i]:offs[i + 1]].view(dt).reshape(h, w, 4).copy() for i, (w, h) in enumerate(sizes)]
    except J40Error as e:
        return e.code, [None] * len(datas)
    finally:
        for f in frames:
            f.close()


SEQ_BLEND = 2   # j40hip_sequence_open's flag J40HIP_SEQ_BLEND: the blend modes Add, Blend, MulAdd and Mul are served
SEQ_LFFRAME = 16   # ... J40HIP_SEQ_LFFRAME: LF frames (type 1) and the frames with use_lf_frame are served
SEQ_COLOUR = 64   # ... J40HIP_SEQ_COLOUR: every handle renders in the colour space the image header signals (Frame.set_colour)
SEQ_PATCHES = 128   # ... J40HIP_SEQ_PATCHES: reference-only frames (type 2) and the frames with a patch dictionary are served
SEQUENCE_PATCHES_FIELDS = ("has_patches", "num_ref", "placements", "slots", "stored_xyb", "xyb_slot", "tiles", "launches")
SEQUENCE_PATCH_FIELDS = ("x", "y", "w", "h", "x0", "y0", "ref", "mode", "clamp", "source")
SEQ_MODULAR_XYB = 32   # ... J40HIP_SEQ_MODULAR_XYB: Modular frames of an XYB image go through the XYB colour tail; with SEQ_LFFRAME a Modular LF frame is served
SEQUENCE_BLEND_FIELDS = ("mode", "alpha_mode", "alpha_chan", "clamp", "alpha_alpha_chan", "alpha_clamp", "src", "blended")
SEQUENCE_FRAME_FIELDS = ("x0", "y0", "w", "h", "duration", "is_last", "shown", "type", "blend", "src", "save_as_reference", "saved",
                         "offset", "end", "first_section", "code", "tps_num", "tps_den", "loops", "canvas_w", "canvas_h")


class Sequence:
    """the coded frames of one codestream -- an animation or a layered still -- and their playback (j40hip_sequence, include/j40hip.h):
    an index over headers and TOCs on the host, every coded frame an ordinary Frame, the displayed canvases composed on the device.
    blend=True (or J40HIP_BLEND=1): frames with the blend modes Add, Blend, MulAdd and Mul are served too, else "TODO" for such a frame.
    lf_frames=True (or J40HIP_LFFRAME=1): LF frames (type 1) and the frames that take their LF image from one (use_lf_frame) are
    served too, else "TODO"; an LF frame is a row that is neither shown nor saved (frame_lf).
    colour=True (or J40HIP_COLOUR=1): every handle renders in the colour space the image header signals (Frame.set_colour): the canvas
    holds pixels in that space, the blend modes work on them as they are.
    modular_xyb=True (or J40HIP_MODULAR_XYB=1): the Modular frames of an XYB image go through the XYB colour tail (Frame.set_modular_xyb);
    together with lf_frames=True a Modular LF frame is served, with either alone it is "TODO".
    patches=True (or J40HIP_PATCHES=1): reference-only frames (type 2, stored as XYB planes in their reference slot, never shown) and
    the frames whose patch dictionary blends rectangles of them onto their own XYB samples are served too, else "TODO" (frame_patches,
    frame_patch, read_ref_slot); a Modular reference-only frame needs modular_xyb=True as well. PARITY UNPINNED.
    noise=True (or J40HIP_NOISE=1): frames with photon noise are served (Frame's noise=); each gets the seed counters of its place in
    the sequence (Frame.noise_params()), so two shown frames get different fields. PARITY UNPINNED.
    splines=True (or J40HIP_SPLINES=1): frames with splines are served (Frame's splines=); a damaged spline stream ("spln") ends the
    index at its frame. PARITY UNPINNED."""

    def __init__(self, data: bytes, threads: int = 4, flags: int = 0, blend: bool = False, wide: bool = False, lf_frames: bool = False, modular_xyb: bool = False, colour: bool = False, patches: bool = False, noise: bool = False, splines: bool = False):
        L = lib()
        self._buf = C.create_string_buffer(data, len(data))
        err = C.c_uint32()
        flags |= (SEQ_BLEND if blend else 0) | (PARSE_WIDE if wide else 0) | (SEQ_LFFRAME if lf_frames else 0) | (SEQ_MODULAR_XYB if modular_xyb else 0) | (SEQ_COLOUR if colour else 0) | (SEQ_PATCHES if patches else 0) | (PARSE_NOISE if noise else 0) | (PARSE_SPLINES if splines else 0)
        self.h = L.j40hip_sequence_open(self._buf, len(data), threads, flags, C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_sequence_open")
        self.num_frames, self.num_shown = int(L.j40hip_sequence_num_frames(self.h)), int(L.j40hip_sequence_num_shown(self.h))
        first = self.frame_info(0)
        self.width, self.height = first["canvas_w"], first["canvas_h"]
        self.tps, self.loops = (first["tps_num"], first["tps_den"]), first["loops"]
        self.fmt = J40_U8X4
        self._lent = []   # (k, weak reference) of every Frame handed out by frame(): their handles die with the sequence's

    def _recall(self, first=0):
        """the Frames handed out for coded frames first.. lose their handles: the sequence is about to free them"""
        for k, ref in self._lent:
            fr = ref()
            if fr is not None and k >= first:
                fr.h = None
        self._lent = [(k, ref) for k, ref in self._lent if k < first and ref() is not None]

    def close(self):
        """frees the sequence and every coded frame's handle; a Frame obtained from frame() is closed with it (its h becomes None)"""
        if self.h:
            self._recall()
            lib().j40hip_sequence_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frame_info(self, k):
        """the index row of coded frame k as a dict (SEQUENCE_FRAME_FIELDS; `code` as text)"""
        out = np.zeros(21, np.int64)
        lib().j40hip_sequence_frame_info(self.h, k, out.ctypes.data)
        d = dict(zip(SEQUENCE_FRAME_FIELDS, out.tolist()))
        d["code"] = err4(d["code"])
        return d

    def frame_blend(self, k):
        """how coded frame k goes onto the canvas, as a dict (SEQUENCE_BLEND_FIELDS): the colour channels' blend mode and the rendered
        alpha channel's, their alpha_chan and clamp, the source slot, whether the frame goes through the blend kernel"""
        out = np.zeros(8, np.int32)
        lib().j40hip_sequence_frame_blend(self.h, k, out.ctypes.data)
        return dict(zip(SEQUENCE_BLEND_FIELDS, out.tolist()))

    def frame_lf(self, k):
        """LF frames: coded frame k's lf_level (0: not an LF frame), use_lf_frame and the row it takes its LF image from (-1: none)"""
        out = np.zeros(4, np.int32)
        lib().j40hip_sequence_frame_lf(self.h, k, out.ctypes.data)
        return {"lf_level": int(out[0]), "use_lf_frame": int(out[1]), "lf_src": int(out[2])}

    def read_lf_slot(self, level, w, h):
        """debug read-back: the picture LF slot level - 1 holds, [3, h, w] float32 (X, Y, B); w x h is the LF frame's size"""
        out = np.zeros((3, h, w), np.float32)
        for c in range(3):
            code = lib().j40hip_sequence_read_lf_slot(self.h, level, c, out[c].ctypes.data)
            if code:
                raise J40Error(err4(code), "in j40hip_sequence_read_lf_slot")
        return out

    def frame_patches(self, k):
        """patches: coded frame k's row as a dict (SEQUENCE_PATCHES_FIELDS) -- whether it has a dictionary, its reference patches and
        placements, the slots they read (a bit mask), whether the row is a reference-only frame stored as XYB planes and in which slot,
        the tiles k_patch_blend gets, and how often the row's handle has launched it"""
        out = np.zeros(8, np.int32)
        lib().j40hip_sequence_frame_patches(self.h, k, out.ctypes.data)
        return dict(zip(SEQUENCE_PATCHES_FIELDS, out.tolist()))

    def frame_patch(self, k, i):
        """placement i (dictionary order) of coded frame k as parsed, as a dict (SEQUENCE_PATCH_FIELDS)"""
        out = np.zeros(10, np.int32)
        code = lib().j40hip_sequence_frame_patch(self.h, k, i, out.ctypes.data)
        if code:
            raise J40Error(err4(code), "in j40hip_sequence_frame_patch")
        return dict(zip(SEQUENCE_PATCH_FIELDS, out.tolist()))

    def read_ref_slot(self, slot):
        """debug read-back: the planes reference slot `slot` holds since a reference-only frame was played into it, [3, h, w] float32 (X, Y, B)"""
        w, h = C.c_int32(), C.c_int32()
        code = lib().j40hip_sequence_ref_slot_size(self.h, slot, C.byref(w), C.byref(h))
        if code:
            raise J40Error(err4(code), "in j40hip_sequence_ref_slot_size")
        out = np.zeros((3, h.value, w.value), np.float32)
        for c in range(3):
            code = lib().j40hip_sequence_read_ref_slot(self.h, slot, c, out[c].ctypes.data)
            if code:
                raise J40Error(err4(code), "in j40hip_sequence_read_ref_slot")
        return out

    def frame(self, k):
        """coded frame k as a Frame the sequence owns: crop-sized, for every single-frame and batch entry point. It lives as long as the
        sequence: close() of the sequence closes it too"""
        err = C.c_uint32()
        h = lib().j40hip_sequence_frame(self.h, k, C.byref(err))
        if not h:
            raise J40Error(err4(err.value), "in j40hip_sequence_frame")
        fr = Frame._borrowed(h, self)
        self._lent.append((k, weakref.ref(fr)))
        return fr

    def upload(self, device=0):
        """every coded frame parsed and uploaded. A frame that does not parse ends the index there (num_frames and num_shown shrink,
        Frames handed out for the rows behind it are closed); the playback reports its code when it gets there"""
        L = lib()
        code = L.j40hip_sequence_upload(self.h, device)
        self.num_frames, self.num_shown = int(L.j40hip_sequence_num_frames(self.h)), int(L.j40hip_sequence_num_shown(self.h))
        self._recall(self.num_frames)
        if code:
            raise J40Error(err4(code), "in j40hip_sequence_upload")

    def set_output_format(self, fmt):
        code = lib().j40hip_sequence_set_output_format(self.h, int(fmt))
        if code:
            raise J40Error(err4(code), "in j40hip_sequence_set_output_format")
        self.fmt = int(fmt)

    def next(self, rgba_ptr, stride_bytes, stream=0):
        """the next displayed canvas into device memory, asynchronously; returns the code as text ("" or "Useq", ...)"""
        return err4(lib().j40hip_sequence_next(self.h, rgba_ptr, stride_bytes, stream))

    def next_to_host(self):
        """(err4, canvas [height, width, 4] or None): the next displayed canvas; "Useq" when none is left"""
        u16 = self.fmt == J40_U16X4
        out = np.zeros((self.height, self.width, 4), np.uint16 if u16 else np.uint8)
        code = err4(lib().j40hip_sequence_next_to_host(self.h, out.ctypes.data, self.width * (8 if u16 else 4)))
        return code, (None if code else out)

    def rewind(self):
        lib().j40hip_sequence_rewind(self.h)

    def status(self):
        """(err4, coded frame) of the first failing section over the frames decoded so far; ("", -1) when there is none"""
        k = C.c_int64(-1)
        code = lib().j40hip_sequence_status(self.h, C.byref(k))
        return err4(code), int(k.value)


def decode_frames(data: bytes, fmt=J40_U8X4, alpha=False, device=0, blend=False, wide=False, lf_frames=False, modular_xyb=False, colour=False, patches=False, noise=False, splines=False):
    """every displayed frame of an animation or a layered still: ([(rgba ndarray [height, width, 4], duration in ticks), ...],
    (tps_num, tps_den, loops)). alpha=True: VarDCT frames keep their alpha channel (Frame.set_alpha(1); J40Error where that refuses).
    blend=True: frames with a blend mode other than Replace are composed too (Sequence's blend=), else such a frame raises "TODO".
    wide=True: an image with 32-bit Modular buffers is served (Sequence's wide=; its Modular frames only).
    lf_frames=True: LF frames and the frames that take their LF image from one are served (Sequence's lf_frames=), else "TODO".
    modular_xyb=True: Modular frames of an XYB image go through the XYB colour tail (Sequence's modular_xyb=).
    colour=True: every frame is rendered in the colour space the image header signals (Sequence's colour=).
    patches=True: reference-only frames and the frames with a patch dictionary are served (Sequence's patches=), else "TODO".
    noise=True: frames with photon noise are served (Sequence's noise=), else "TODO".
    splines=True: frames with splines are served (Sequence's splines=), else "TODO".
    A frame that fails raises J40Error with its code. A stream whose first frame is its last is not a sequence ("Usq?"): decode()."""
    seq = Sequence(data, blend=blend, wide=wide, lf_frames=lf_frames, modular_xyb=modular_xyb, colour=colour, patches=patches, noise=noise, splines=splines)
    try:
        seq.set_output_format(fmt)
        if alpha:
            for k in range(seq.num_frames):
                code = seq.frame(k).set_alpha(1)
                if code:
                    raise J40Error(code, "in j40hip_frame_set_alpha")
        seq.upload(device)
        durations = [seq.frame_info(k)["duration"] for k in range(seq.num_frames) if seq.frame_info(k)["shown"]]
        frames = []
        while True:
            code, px = seq.next_to_host()
            if code == "Useq":
                break
            if code:
                raise J40Error(code, "in j40hip_sequence_next_to_host")
            frames.append((px, durations[len(frames)]))
        return frames, (seq.tps[0], seq.tps[1], seq.loops)
    finally:
        seq.close()


class Batch:
    """throughput mode (include/j40hip.h, j40hip_batch_*): uploaded VarDCT frames decoded by one entropy
    launch with one pass-group section per wavefront lane"""

    def __init__(self, frames):
        L = lib()
        self.frames = list(frames)
        arr = (C.c_void_p * len(self.frames))(*[f.h for f in self.frames])
        err = C.c_uint32()
        self.h = L.j40hip_batch_create(arr, len(self.frames), C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_batch_create")

    def close(self):
        if self.h:
            lib().j40hip_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _args(self, rgba_ptrs, strides):
        n = len(self.frames)
        return (C.c_void_p * n)(*rgba_ptrs), (C.c_size_t * n)(*strides)

    def decode(self, rgba_ptrs, strides, stream=0):
        p, s = self._args(rgba_ptrs, strides)
        code = lib().j40hip_batch_decode(self.h, p, s, stream)
        if code:
            raise J40Error(err4(code), "in j40hip_batch_decode")

    def decode_recorded(self, rgba_ptrs, strides, stream, slot):
        """asynchronous: stage events go to `slot`; read them with elapsed(slot) after synchronising the stream"""
        p, s = self._args(rgba_ptrs, strides)
        code = lib().j40hip_batch_decode_recorded(self.h, p, s, stream, slot)
        if code:
            raise J40Error(err4(code), "in j40hip_batch_decode_recorded")

    def wait_stage(self, slot, stage, stream):
        """`stream` waits for stage 1 (cleared) / 2 (entropy decoded) / 3 (pixels written) of the decode recorded in `slot`"""
        code = lib().j40hip_batch_wait_stage(self.h, slot, stage, stream)
        if code:
            raise J40Error(err4(code), "in j40hip_batch_wait_stage")

    def elapsed(self, slot):
        ms = (C.c_float * 3)()
        code = lib().j40hip_batch_elapsed(self.h, slot, ms)
        if code:
            raise J40Error(err4(code), "in j40hip_batch_elapsed")
        return ms[0], ms[1], ms[2]

    def decode_timed(self, rgba_ptrs, strides, stream=0):
        """returns (entropy ms, pixels ms, clear ms) measured with HIP events on `stream`"""
        p, s = self._args(rgba_ptrs, strides)
        ms = (C.c_float * 3)()
        code = lib().j40hip_batch_decode_timed(self.h, p, s, stream, ms)
        if code:
            raise J40Error(err4(code), "in j40hip_batch_decode_timed")
        return ms[0], ms[1], ms[2]


class StageDump:
    """j40hip_stage_dump_*: one image through the pipeline's device stages, every stage's product copied back (parity tests)"""

    def __init__(self, data, device=0, lf_on_device=True):
        self._buf = C.create_string_buffer(bytes(data), len(data))
        err = C.c_uint32()
        self.h = lib().j40hip_stage_dump_create(self._buf, len(data), device, 1 if lf_on_device else 0, C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_stage_dump_create")
        a = np.zeros(8, np.uint32)
        lib().j40hip_stage_dump_info(self.h, a.ctypes.data)
        self.verdict, self.flags = err4(int(a[0])), int(a[1])
        self.lf_on_device = bool(a[1] & 4)
        self.num_lf_groups, self.num_groups, self.width, self.height, self.dct_used, self.num_varblocks = (int(v) for v in a[2:8])

    def lf_group_info(self, gg):
        a = np.zeros(10, np.int32)
        assert lib().j40hip_stage_dump_lf_group_info(self.h, gg, a.ctypes.data) == 0
        d = dict(zip(["left", "top", "width", "height", "width8", "height8", "width64", "height64", "nb_varblocks"], a[:9].tolist()))
        d["status"] = err4(int(a[9]) & 0xffffffff)
        return d

    def plane(self, gg, which):
        gi = self.lf_group_info(gg)
        c8, c64 = (gi["height8"], gi["width8"]), (gi["height64"], gi["width64"])
        shape, dt = {0: (c8, np.int32), 1: (c8, np.uint8), 2: (c64, np.int16), 3: (c64, np.int16), 4: (c8, np.int16), 5: (c8, np.int16), 6: (c8, np.int16), 7: (c8, np.int16)}[which]
        a = np.zeros(shape, dt)
        if lib().j40hip_stage_dump_plane(self.h, gg, which, a.ctypes.data) != 0:
            return None
        return a

    def varblocks(self, gg):
        n = self.lf_group_info(gg)["nb_varblocks"]
        a, b, c = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 3), np.int32)
        assert lib().j40hip_stage_dump_varblocks(self.h, gg, a.ctypes.data, b.ctypes.data, c.ctypes.data) == n
        return a[:n], b[:n], c[:n]

    def llf(self, gg, c):
        gi = self.lf_group_info(gg)
        a = np.zeros(gi["height8"] * gi["width8"], np.float32)
        assert lib().j40hip_stage_dump_llf(self.h, gg, c, a.ctypes.data) == 0
        return a

    def group_blocks(self, group):
        a = np.zeros((1024, 3), np.uint32)
        n = lib().j40hip_stage_dump_group_blocks(self.h, group, a.ctypes.data, 1024)
        assert 0 <= n <= 1024
        return a[:n]

    def sorted_varblocks(self):
        cap = max(self.num_varblocks, 1)
        a, f, cs = np.zeros((cap, 8), np.int32), np.zeros((cap, 3), np.float32), np.zeros(28, np.int32)
        n = lib().j40hip_stage_dump_sorted_varblocks(self.h, a.ctypes.data, f.ctypes.data, cs.ctypes.data, cap)
        assert 0 <= n <= cap
        return a[:n], f[:n], cs

    def rgba(self):
        a = np.zeros((self.height, self.width, 4), np.uint8)
        assert lib().j40hip_stage_dump_rgba(self.h, a.ctypes.data) == 0
        return a

    def close(self):
        if self.h:
            lib().j40hip_stage_dump_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """whole-frame throughput pipeline (include/j40hip.h, j40hip_pipeline_*): codestreams in host memory -> RGBA u8x4 in host or
    device memory; host worker threads parse and upload, one thread batches the uploaded frames per entropy launch"""

    def __init__(self, device=0, host_threads=0, batch_frames=32, max_in_flight=2, lf_streams="auto", tune_malloc=False, lf_on_device=None):
        """lf_streams: who decodes the LfGroup streams of the batched frames -- "auto" (decided frame by frame), "device"
        (k_lf_lanes), "host" (the worker threads). `lf_on_device` is the deprecated spelling of rounds 1-2: True = "device",
        False = "host"."""
        if lf_on_device is not None:
            lf_streams = "device" if lf_on_device else "host"
        err = C.c_uint32()
        flags = {"auto": 0, "device": 1, "host": 2}[lf_streams] | (4 if tune_malloc else 0)
        self.h = lib().j40hip_pipeline_create_ex(device, host_threads, batch_frames, max_in_flight, flags, C.byref(err))
        if not self.h:
            raise J40Error(err4(err.value), "in j40hip_pipeline_create")
        self._keep = []

    def lf_device_frames(self):
        return int(lib().j40hip_pipeline_lf_device_frames(self.h))

    def submit(self, data, rgba_ptr, stride_bytes, device_output=False):
        """data: bytes-like (kept alive until close / drain); rgba_ptr: address of the output image; returns the ticket"""
        buf = data if isinstance(data, C.Array) else C.create_string_buffer(bytes(data), len(data))
        self._keep.append(buf)
        t = C.c_int64()
        code = lib().j40hip_pipeline_submit(self.h, buf, len(data), rgba_ptr, stride_bytes, 1 if device_output else 0, C.byref(t))
        if code:
            raise J40Error(err4(code), "in j40hip_pipeline_submit")
        return t.value

    def submit_raw(self, buf, size, rgba_ptr, stride_bytes, device_output=False):
        """as submit, for a ctypes buffer the caller keeps alive until the ticket is done"""
        t = C.c_int64()
        code = lib().j40hip_pipeline_submit(self.h, buf, size, rgba_ptr, stride_bytes, 1 if device_output else 0, C.byref(t))
        if code:
            raise J40Error(err4(code), "in j40hip_pipeline_submit")
        return t.value

    def run(self, data):
        """one image, synchronously (j40hip_pipeline_run): the calling thread sleeps until it is done; any number of threads may call
        this at once and share the pipeline's batches. Returns (err4, rgba ndarray [height, width, 4] or None)."""
        buf = data if isinstance(data, C.Array) else C.create_string_buffer(bytes(data), len(data))
        got = {}

        def alloc(ctx, width, height, stride_out):
            got["a"] = np.empty((int(height), int(width), 4), np.uint8)
            stride_out[0] = int(width) * 4
            return got["a"].ctypes.data

        cb = OUTPUT_ALLOC(alloc)
        code = lib().j40hip_pipeline_run(self.h, buf, len(data), cb, None)
        return err4(code), (got.get("a") if not code else None)

    def set_scale(self, shift):
        """every image submitted afterwards comes out at 1:2 (1) or 1:4 (2): rgba / stride_bytes of submit, and the arrays run
        returns, are the small image's (j40hip_pipeline_set_scale). Returns "" or "rnge" / "Usc?" (images in flight: drain first)"""
        return err4(lib().j40hip_pipeline_set_scale(self.h, int(shift)))

    def set_max_wait_ms(self, ms):
        lib().j40hip_pipeline_set_max_wait_ms(self.h, float(ms))

    def drain(self):
        code = lib().j40hip_pipeline_drain(self.h)
        if code:
            raise J40Error(err4(code), "in j40hip_pipeline_drain")
        self._keep = []

    def result(self, ticket):
        return err4(lib().j40hip_pipeline_result(self.h, ticket))

    def stats(self):
        a = (C.c_double * 12)()
        lib().j40hip_pipeline_stats_ex(self.h, a)
        # (upload_thread_ms: single_thread_ms under the name it had until round 3)
        b = (C.c_double * 5)()
        lib().j40hip_pipeline_lf_stats(self.h, b)
        return dict(parse_thread_ms=a[0], single_thread_ms=a[1], upload_thread_ms=a[1], completed=int(a[2]), wall_ms=a[3], k1_ms=a[4], k2_ms=a[5], launches=int(a[6]), launch_frames=int(a[7]),
                    lf_plan_ms=a[8], lf_device_frames=int(a[9]), single_frames=int(a[10]), k1_kernel_ms=a[11],
                    lf_kernel_ms=b[0], lf_launches=int(b[1]), lf_launch_frames=int(b[2]), lf_launch_sections=int(b[3]), lf_launch_waves=int(b[4]))

    def reset_stats(self):
        lib().j40hip_pipeline_reset_stats(self.h)

    def close(self):
        if self.h:
            lib().j40hip_pipeline_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
