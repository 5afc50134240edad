"""ctypes binding of lib/libtendrils_hip.so (the C ABI in include/tendrils_hip.h).

This is plumbing: every symbol the header declares is bound here, nothing is
computed in Python.  There is no CPU fallback - if the library is missing or no
gfx950 device is present, calls raise.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TH_LIB") or os.path.join(HERE, "lib", "libtendrils_hip.so")   # TH_LIB: diagnostic builds

TH_OK = 0
TH_MODE_EXACT, TH_MODE_FAST = 0, 1
TH_STATE_F32, TH_STATE_F16 = 0, 1
TH_PASS_FLOW, TH_PASS_VIEW = 0, 1
TH_MAX_LINE_WIDTH = 64.0
TH_TARGET_RING, TH_TARGET_TARGETS, TH_SOURCE_FLOW, TH_SOURCE_IMAGE, TH_SOURCE_NONE = -1, -2, -3, -4, -5
TH_ERR_INVALID, TH_ERR_HIP, TH_ERR_NO_DEVICE, TH_ERR_UNSUPPORTED = 1, 2, 3, 4
INERT = -1000000.0


class TendrilsHipError(RuntimeError):
    """A C-ABI call returned a non-zero status (the reference throws JS Errors from gl-fbo/gl-shader)."""

    def __init__(self, status, message):
        super().__init__("tendrils_hip status %d: %s" % (status, message))
        self.status = status


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("global_height", C.c_int32), ("row0", C.c_int32), ("num_buffers", C.c_int32),
                ("mode", C.c_int32), ("state_format", C.c_int32)]


class LogicUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2),
                ("time", C.c_float), ("dt", C.c_float),
                ("speedLimit", C.c_float), ("damping", C.c_float),
                ("forceWeight", C.c_float), ("flowWeight", C.c_float), ("noiseWeight", C.c_float),
                ("flowDecay", C.c_float),
                ("noiseSpeed", C.c_float), ("noiseScale", C.c_float),
                ("target", C.c_float),
                ("varyForce", C.c_float), ("varyFlow", C.c_float), ("varyNoise", C.c_float),
                ("varyNoiseScale", C.c_float), ("varyNoiseSpeed", C.c_float), ("varyTarget", C.c_float)]


class OpticalFlowUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("scaleUV", C.c_float * 2),
                ("offset", C.c_float), ("lambda_", C.c_float),
                ("time", C.c_float), ("speed", C.c_float), ("speedLimit", C.c_float)]


class SpawnBallUniforms(C.Structure):
    _fields_ = [("radius", C.c_float), ("speed", C.c_float)]


class SpawnSampleUniforms(C.Structure):
    _fields_ = [("spawnSize", C.c_float * 2), ("jitter", C.c_float * 2),
                ("time", C.c_float), ("speed", C.c_float), ("bias", C.c_float),
                ("flowDecay", C.c_float),
                ("spawnMatrix", C.c_float * 9),
                ("samples", C.c_int32), ("apply", C.c_int32)]


class DepositUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("time", C.c_float), ("speedLimit", C.c_float)]


class Counters(C.Structure):
    _fields_ = [("particles", C.c_uint64), ("live", C.c_uint64), ("nan", C.c_uint64),
                ("capped", C.c_uint64), ("respawned", C.c_uint64),
                ("sum_speed", C.c_double), ("max_speed", C.c_double)]


class RenderUniforms(C.Structure):
    _fields_ = [("viewSize", C.c_float * 2), ("time", C.c_float), ("speedLimit", C.c_float), ("flowDecay", C.c_float),
                ("speedAlpha", C.c_float), ("colorMapAlpha", C.c_float), ("sinTerm", C.c_float),
                ("baseColor", C.c_float * 4), ("flowColor", C.c_float * 4)]


class ShapesInfo(C.Structure):
    _fields_ = [("state_w", C.c_int32), ("state_h", C.c_int32), ("flow_w", C.c_int32), ("flow_h", C.c_int32),
                ("frames_w", C.c_int32), ("frames_h", C.c_int32)]


class SlotOrderInfo(C.Structure):
    _fields_ = [("sorted_buffers", C.c_int32), ("steps_since_sort", C.c_int32), ("window_misses", C.c_uint64),
                ("sorts", C.c_uint64)]


class DrawInfo(C.Structure):
    _fields_ = [("pipeline", C.c_int32), ("reserved", C.c_int32), ("fragments", C.c_uint64), ("crowded_fragments", C.c_uint64),
                ("sent_bytes", C.c_uint64), ("received_bytes", C.c_uint64)]


class SpawnInfo(C.Structure):
    _fields_ = [("taps", C.c_uint64), ("local_taps", C.c_uint64), ("sent_bytes", C.c_uint64), ("received_bytes", C.c_uint64),
                ("chunks", C.c_int32), ("reserved", C.c_int32)]


class CommInfo(C.Structure):
    _fields_ = [("active", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("rccl_version", C.c_int32)]


class ProgramInfo(C.Structure):
    _fields_ = [("vgprs", C.c_uint32), ("sgprs", C.c_uint32), ("lds_bytes", C.c_uint32), ("scratch_bytes", C.c_uint32),
                ("code_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class MeasureResult(C.Structure):
    """th_measure_result: what a measure program's reduction returns (144 bytes)"""
    _fields_ = [("taken", C.c_uint64), ("particles", C.c_uint64), ("sum", C.c_double * 8), ("min", C.c_float * 8),
                ("max", C.c_float * 8)]


class DensityUniforms(C.Structure):
    """th_density_uniforms: the view size, the grid and where the image goes (24 bytes)"""
    _fields_ = [("viewSize", C.c_float * 2), ("w", C.c_int32), ("h", C.c_int32), ("dest", C.c_int32), ("slot", C.c_int32)]


class DensityInfo(C.Structure):
    """th_density_info: what a density call says of the particles it went over (40 bytes)"""
    _fields_ = [("particles", C.c_uint64), ("live", C.c_uint64), ("inside", C.c_uint64), ("outside", C.c_uint64),
                ("nonfinite_velocity", C.c_uint64)]


SELECT_BOX, SELECT_SPEED, SELECT_INERT = 1, 2, 4           # TH_SELECT_*


class SelectUniforms(C.Structure):
    """th_select_uniforms: the box, the squared speeds, the thinning and which clauses count (40 bytes)"""
    _fields_ = [("box", C.c_float * 4), ("speed2", C.c_float * 2), ("stride", C.c_uint32), ("phase", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Selected(C.Structure):
    """th_selected: one matching particle - its state as decoded, its texel in the whole texture (32 bytes)"""
    _fields_ = [("state", C.c_float * 4), ("index", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("reserved", C.c_uint32)]


class SelectInfo(C.Structure):
    """th_select_info: what a select says of the particles it went over (32 bytes)"""
    _fields_ = [("particles", C.c_uint64), ("live", C.c_uint64), ("matched", C.c_uint64), ("written", C.c_uint64)]


HIST_X, HIST_Y, HIST_VX, HIST_VY, HIST_SPEED2, HIST_SPEED = range(6)      # TH_HIST_*: the channel
HIST_LINEAR, HIST_KEY = 0, 1                               # ... the mode
HIST_MAX_BINS = 4096


class HistogramUniforms(C.Structure):
    """th_histogram_uniforms: which particles (a th_select_uniforms), which scalar, how it is binned (72 bytes)"""
    _fields_ = [("select", SelectUniforms), ("channel", C.c_int32), ("mode", C.c_int32), ("bins", C.c_uint32),
                ("lo", C.c_float), ("hi", C.c_float), ("key_prefix", C.c_uint32), ("key_shift", C.c_uint32), ("reserved", C.c_uint32)]


class HistogramInfo(C.Structure):
    """th_histogram_info: what a histogram says of the particles it went over (48 bytes)"""
    _fields_ = [("particles", C.c_uint64), ("live", C.c_uint64), ("matched", C.c_uint64), ("below", C.c_uint64),
                ("above", C.c_uint64), ("nan", C.c_uint64)]


FOLLOW_MAX_PARTICLES, FOLLOW_MAX_DEPTH, FOLLOW_MAX_ENTRIES = 1 << 20, 1 << 16, 1 << 24      # TH_FOLLOW_MAX_*


class FollowInfo(C.Structure):
    """th_follow_info: the followed set, its history and how often its slots were found again (48 bytes)"""
    _fields_ = [("particles", C.c_uint64), ("followed", C.c_uint64), ("depth", C.c_uint64), ("samples", C.c_uint64),
                ("held", C.c_uint64), ("locates", C.c_uint64)]


class DrawStages(C.Structure):
    """th_draw_stages: a draw program or None (the library's vertex stage, with `builtin` its uniforms), a fragment program or None"""
    _fields_ = [("vertex", C.c_void_p), ("vertex_uniforms", C.c_void_p), ("vertex_uniform_bytes", C.c_uint32),
                ("fragment", C.c_void_p), ("fragment_uniforms", C.c_void_p), ("fragment_uniform_bytes", C.c_uint32),
                ("builtin", C.c_void_p)]


class FlowLineUniforms(C.Structure):
    _fields_ = [("speed", C.c_float), ("rad", C.c_float), ("crestShape", C.c_float), ("speedLimit", C.c_float),
                ("viewSize", C.c_float * 2)]


class BlendView(C.Structure):
    _fields_ = [("source", C.c_int32), ("index", C.c_int32), ("alpha", C.c_float)]


class ScreenUnit(C.Structure):
    _fields_ = [("source", C.c_int32), ("index", C.c_int32)]


COMM_ID_BYTES = 128         # TH_COMM_ID_BYTES
TEX_RGBA32F, TEX_RGBA8, TEX_L32F = 0, 1, 2                  # TH_TEX_*
VIEW_TEXTURE, VIEW_FRAMES, VIEW_SPAWN_IMAGE = 0, 1, 2       # TH_VIEW_*
VIEW_BUFFER, VIEW_SCREEN, VIEW_COLORMAP, VIEW_FLOW = 3, 4, 5, 6      # ... th_screen_run alone
SCREEN_TARGET_VIEW, SCREEN_TARGET_COLORMAP, SCREEN_TARGET_TEXTURE = 0, 1, 2      # TH_SCREEN_TARGET_*
MAX_TEXTURES = MAX_BLEND_VIEWS = 8                          # TH_MAX_TEXTURES, TH_MAX_BLEND_VIEWS

_ctx = C.c_void_p
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); mirrors include/tendrils_hip.h one to one
PROTOTYPES = {
    "th_abi_version": (C.c_int32, []),
    "th_last_error": (C.c_char_p, []),
    "th_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "th_create": (C.c_int32, [C.POINTER(Config), C.POINTER(_ctx)]),
    "th_destroy": (C.c_int32, [_ctx]),
    "th_set_mode": (C.c_int32, [_ctx, C.c_int32]),
    "th_setup": (C.c_int32, [_ctx, C.c_int32]),
    "th_num_buffers": (C.c_int32, [_ctx, C.POINTER(C.c_int32)]),
    "th_upload_state": (C.c_int32, [_ctx, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "th_download_state": (C.c_int32, [_ctx, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "th_flow_resize": (C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    "th_flow_upload": (C.c_int32, [_ctx, _fp]),
    "th_flow_download": (C.c_int32, [_ctx, _fp]),
    "th_flow_clear": (C.c_int32, [_ctx]),
    "th_targets_upload": (C.c_int32, [_ctx, _fp]),
    "th_targets_download": (C.c_int32, [_ctx, _fp]),
    "th_targets_clear": (C.c_int32, [_ctx]),
    "th_step": (C.c_int32, [_ctx, C.POINTER(LogicUniforms), C.c_int32]),
    "th_step_n": (C.c_int32, [_ctx, C.POINTER(LogicUniforms), C.c_double, C.c_double, C.c_int32]),
    "th_spawn_init": (C.c_int32, [_ctx, C.c_int32]),
    "th_spawn_ball": (C.c_int32, [_ctx, C.POINTER(SpawnBallUniforms), C.c_int32]),
    "th_spawn_sample": (C.c_int32, [_ctx, C.POINTER(SpawnSampleUniforms), C.c_int32, C.c_int32]),
    "th_spawn_direct": (C.c_int32, [_ctx, C.POINTER(SpawnSampleUniforms), C.c_int32, C.c_int32]),
    "th_spawn_image_upload": (C.c_int32, [_ctx, _fp, C.c_int32, C.c_int32]),
    "th_spawn_image_triangles": (C.c_int32, [_ctx, _fp, C.c_int32, _fp, _fp, C.c_int32, C.c_int32]),
    "th_spawn_image_download": (C.c_int32, [_ctx, _fp]),
    "th_frames_resize": (C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    "th_frames_upload": (C.c_int32, [_ctx, C.POINTER(C.c_uint8)]),
    "th_frames_rotate": (C.c_int32, [_ctx]),
    "th_optical_flow": (C.c_int32, [_ctx, C.POINTER(OpticalFlowUniforms)]),
    "th_flow_deposit": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), C.POINTER(C.c_uint64)]),
    "th_export_lines": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), _fp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "th_deposit_emit": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_deposit_set_halo": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p]),
    "th_deposit_set_owners": (C.c_int32, [_ctx, C.c_int32]),
    "th_deposit_merge": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint64]),
    "th_flow_device_ptr": (C.c_int32, [_ctx, C.POINTER(C.c_void_p)]),
    "th_view_emit": (C.c_int32, [_ctx, C.POINTER(RenderUniforms), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_view_merge": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint64]),
    "th_draw_emit": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), C.POINTER(RenderUniforms), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_draw_merge": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint64]),
    "th_draw_sharded": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), C.POINTER(RenderUniforms), C.POINTER(C.c_uint64)]),
    "th_view_device_ptr": (C.c_int32, [_ctx, C.POINTER(C.c_void_p)]),
    "th_state_gather": (C.c_int32, [_ctx, C.c_int32]),
    "th_state_gather_ptr": (C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_void_p)]),
    "th_spawn_sample_sharded": (C.c_int32, [_ctx, C.POINTER(SpawnSampleUniforms), C.c_int32, C.c_int32]),
    "th_spawn_query": (C.c_int32, [_ctx, C.POINTER(SpawnInfo)]),
    "th_stats": (C.c_int32, [_ctx, C.c_float, C.POINTER(Counters)]),
    "th_stats_async": (C.c_int32, [_ctx, C.c_float, C.POINTER(C.c_void_p)]),
    "th_comm_unique_id": (C.c_int32, [C.c_void_p]),
    "th_comm_loopback_id": (C.c_int32, [C.c_void_p]),
    "th_comm_init": (C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32]),
    "th_comm_destroy": (C.c_int32, [_ctx]),
    "th_comm_query": (C.c_int32, [_ctx, C.POINTER(CommInfo)]),
    "th_stats_allreduce": (C.c_int32, [_ctx]),
    "th_stats_global": (C.c_int32, [_ctx, C.c_float, C.POINTER(Counters)]),
    "th_sync": (C.c_int32, [_ctx]),
    "th_stream": (C.c_int32, [_ctx, C.POINTER(C.c_void_p)]),
    "th_state_device_ptr": (C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_void_p)]),
    "th_timer_start": (C.c_int32, [_ctx]),
    "th_timer_stop": (C.c_int32, [_ctx, C.POINTER(C.c_float)]),
    "th_kernel_timing": (C.c_int32, [_ctx, C.c_int32]),
    "th_kernel_timing_read": (C.c_int32, [_ctx, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "th_slot_order": (C.c_int32, [_ctx, C.POINTER(SlotOrderInfo)]),
    "th_slot_order_read": (C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                       C.c_void_p, C.POINTER(C.c_int32)]),
    "th_shapes": (C.c_int32, [_ctx, C.POINTER(ShapesInfo)]),
    "th_draw_pipeline": (C.c_int32, [_ctx, C.c_int32]),
    "th_draw_query": (C.c_int32, [_ctx, C.POINTER(DrawInfo)]),
    "th_option_set": (C.c_int32, [_ctx, C.c_int32, C.c_int64]),
    "th_option_get": (C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_int64)]),
    "th_line_width": (C.c_int32, [_ctx, C.c_int32, C.c_float]),
    "th_line_width_range": (C.c_int32, [_ctx, C.c_float, C.c_float]),
    "th_line_width_query": (C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "th_view_draw": (C.c_int32, [_ctx, C.POINTER(RenderUniforms), C.POINTER(C.c_uint64)]),
    "th_draw": (C.c_int32, [_ctx, C.POINTER(DepositUniforms), C.POINTER(RenderUniforms), C.POINTER(C.c_uint64)]),
    "th_view_fill": (C.c_int32, [_ctx, _fp]),
    "th_view_clear": (C.c_int32, [_ctx]),
    "th_view_download": (C.c_int32, [_ctx, C.POINTER(C.c_uint8)]),
    "th_view_buffers": (C.c_int32, [_ctx, C.c_int32]),
    "th_view_bind": (C.c_int32, [_ctx, C.c_int32]),
    "th_view_copy": (C.c_int32, [_ctx, C.c_int32]),
    "th_view_step_buffers": (C.c_int32, [_ctx]),
    "th_colormap_upload": (C.c_int32, [_ctx, _fp, C.c_int32, C.c_int32]),
    "th_texture_upload": (C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "th_texture_download": (C.c_int32, [_ctx, C.c_int32, C.c_void_p]),
    "th_colormap_resize": (C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    "th_colormap_shape": (C.c_int32, [_ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "th_colormap_blend": (C.c_int32, [_ctx, C.POINTER(BlendView), C.c_int32, C.c_int32, C.c_int32]),
    "th_colormap_download": (C.c_int32, [_ctx, _fp]),
    "th_export_view_lines": (C.c_int32, [_ctx, C.POINTER(RenderUniforms), _fp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "th_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "th_program_log": (C.c_char_p, []),
    "th_program_destroy": (C.c_int32, [C.c_void_p]),
    "th_program_run": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32]),
    "th_program_query": (C.c_int32, [_ctx, C.c_void_p, C.POINTER(ProgramInfo)]),
    "th_screen_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "th_screen_run": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ScreenUnit), C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32]),
    "th_draw_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "th_draw_program_run": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64)]),
    "th_draw_program_emit": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]),
    "th_draw_program_sharded": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(DepositUniforms),
                                            C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RenderUniforms),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "th_fragment_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "th_draw_stages_run": (C.c_int32, [_ctx, C.POINTER(DrawStages), C.c_int32, C.POINTER(C.c_uint64)]),
    "th_draw_stages_emit": (C.c_int32, [_ctx, C.POINTER(DrawStages), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p)]),
    "th_draw_stages_pair": (C.c_int32, [_ctx, C.POINTER(DrawStages), C.POINTER(DrawStages), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "th_step_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "th_step_program_run": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_float), C.c_float, C.c_int32]),
    "th_step_program_view_size": (C.c_int32, [_ctx, C.POINTER(C.c_float)]),
    "th_measure_program_compile": (C.c_int32, [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "th_measure_run": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(MeasureResult)]),
    "th_measure_async": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "th_measure_global": (C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(MeasureResult)]),
    "th_density": (C.c_int32, [_ctx, C.POINTER(DensityUniforms), C.c_int32, C.POINTER(DensityInfo)]),
    "th_density_async": (C.c_int32, [_ctx, C.POINTER(DensityUniforms), C.c_int32, C.POINTER(C.c_void_p)]),
    "th_select": (C.c_int32, [_ctx, C.POINTER(SelectUniforms), C.c_int32, C.POINTER(Selected), C.c_uint64, C.POINTER(SelectInfo)]),
    "th_select_async": (C.c_int32, [_ctx, C.POINTER(SelectUniforms), C.c_int32, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_histogram": (C.c_int32, [_ctx, C.POINTER(HistogramUniforms), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(HistogramInfo)]),
    "th_histogram_async": (C.c_int32, [_ctx, C.POINTER(HistogramUniforms), C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_follow_set": (C.c_int32, [_ctx, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32]),
    "th_follow_sample": (C.c_int32, [_ctx, C.c_int32, C.c_double]),
    "th_follow_read": (C.c_int32, [_ctx, C.c_uint64, C.c_uint64, _fp, C.POINTER(C.c_double), C.POINTER(FollowInfo)]),
    "th_follow_query": (C.c_int32, [_ctx, C.POINTER(FollowInfo), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "th_flow_line_attributes": (C.c_int32, [_fp, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                            _fp, _fp, _fp, _fp, _fp, _fp]),
    "th_flow_lines": (C.c_int32, [_ctx, C.POINTER(FlowLineUniforms), _fp, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), C.c_int32]),
}

_NO_STATUS = {"th_abi_version", "th_last_error", "th_program_log"}
TEST_BUILD_ONLY = {"th_comm_loopback_id"}      # declared under TH_TESTING in include/tendrils_hip.h
_lib = None


def _mapped(name):
    """paths of the shared objects called `name`* that this process has mapped"""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(" ", 1)[-1].strip()
                if os.path.basename(path).startswith(name):
                    found.add(os.path.realpath(path))
    except OSError:
        pass
    return found


def _runtime_order():
    """PyTorch-ROCm wheels bundle their own ROCm runtime (libamdhip64 / libhsa-runtime64 under torch/lib); this library
    links the system one.  A process must end up with ONE runtime: the copy that is mapped first serves everybody
    (same SONAMEs), and that only works in one order - torch's first (the other way round torch finds no devices).  So
    when torch is installed it is imported before the library is loaded, whatever the caller's import order was;
    TH_SKIP_TORCH=1 skips that (hosts that never touch torch)."""
    import importlib.util
    import sys
    if os.environ.get("TH_SKIP_TORCH") == "1" or "torch" in sys.modules:
        return
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load():
    """Load the shared library (raises OSError if it was not built) and bind every symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not found - run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C tendrils_amd/csrc)" % LIB_PATH)
        _runtime_order()
        lib = C.CDLL(LIB_PATH)
        # (a profiler's preloaded tool library maps the system runtime before Python starts: not this loader's doing)
        profiled = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ)
        paths = _mapped("libamdhip64")
        import sys
        if len(paths) > 1 and not profiled and "torch" not in sys.modules:
            # (a host that never touches torch shares no streams with it: two copies on disk under different names -
            # a hashed wheel copy, another ROCm - are this host's own business)
            import warnings
            warnings.warn("two copies of the HIP runtime are mapped into this process: %s" % ", ".join(sorted(paths)))
        elif len(paths) > 1 and not profiled:
            raise OSError("two copies of the HIP runtime are mapped into this process (%s): streams and events cannot be "
                          "shared between them - import torch before anything loads the ROCm runtime, or set "
                          "TH_SKIP_TORCH=1 and keep torch out of the process" % ", ".join(sorted(paths)))
        for name, (res, args) in PROTOTYPES.items():
            if name in TEST_BUILD_ONLY and not hasattr(lib, name):
                continue                 # a release build of the library (make release): the test machinery is not in it
            fn = getattr(lib, name)      # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def call(name, *args):
    """Invoke a status-returning entry point; raise TendrilsHipError on failure."""
    lib = load()
    status = getattr(lib, name)(*args)
    if name not in _NO_STATUS and status != TH_OK:
        raise TendrilsHipError(status, lib.th_last_error().decode(errors="replace"))
    return status
