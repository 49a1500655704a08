"""ctypes binding of include/multifm_hip.h (libmultifm_hip.so).

Used by tests/, bench.py and __graft_entry__.py.  It is a thin mirror of the C ABI: one Python
method per entry point, errors raised as MfmError carrying the library's message.  There is no
fallback: if the shared library is missing, importing the engine fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFM_LIB") or os.path.join(_HERE, "libmultifm_hip.so")

MFM_OK, MFM_E_INVAL, MFM_E_NOMEM, MFM_E_BUSY, MFM_E_DEVICE, MFM_E_STATE, MFM_E_DONE = 0, -1, -2, -3, -4, -5, -6
MFM_ABI_VERSION = 4
MFM_F_DEVICE_ONLY = 0x1
MFM_F_TIMING = 0x2
MFM_F_FORCE_DOT2 = 0x4
MFM_F_FORCE_MFMA_V1 = 0x8
MFM_F_WIDEN_8BIT = 0x10
MFM_F_TIMING_SPARSE = 0x20
MFM_F_GROUP_SHARED_DEVICE = 0x40
MFM_F_STREAM_TAPS = 0x80
MFM_F_GATHER = 0x100
MFM_F_OVERLAP = 0x200
MFM_F_V3L_ONE_ROW_BLOCK = 0x400
MFM_F_SLICE_128 = 0x800
MFM_F_SLICE_64 = 0x1000
MFM_F_PCM_WRITE_BACK = 0x2000
MFM_RCP_TABLE_HASH_GFX950 = 0x706D94BC005BCC1A  # include/multifm_hip.h
MFM_IN_CS16, MFM_IN_CS8, MFM_IN_CU8, MFM_IN_RTLSDR_U8 = 0, 1, 2, 3
MFM_BITS_NEG, MFM_BITS_POS = 1, 2  # sign-bit views: bit = sample < 0 (POCSAG) / sample > 0 (AIS)

# every symbol include/multifm_hip.h declares (tests check the library exports each one)
ABI_SYMBOLS = [
    "mfm_engine_input_bytes", "mfm_engine_input_bytes_cfg", "mfm_engine_flush", "mfm_engine_replay", "mfm_group_flush",
    "mfm_engine_last_launch_input", "mfm_engine_seek", "mfm_devtest_discriminate", "mfm_devtest_rcp_table",
    "mfm_host_alloc", "mfm_host_free", "mfm_engine_push_pinned", "mfm_engine_copy_done", "mfm_engine_copy_wait",
    "mfm_group_push_pinned", "mfm_group_copy_done", "mfm_group_copy_wait", "mfm_group_replay_pinned",
    "mfm_engine_create", "mfm_engine_destroy", "mfm_engine_add_channel",
    "mfm_engine_add_channel_q14", "mfm_engine_get_channel", "mfm_engine_commit", "mfm_engine_acquire_input",
    "mfm_engine_acquire_input_bytes",
    "mfm_engine_submit", "mfm_engine_push", "mfm_engine_push_bytes", "mfm_engine_fetch", "mfm_engine_release",
    "mfm_engine_last_output_device", "mfm_engine_sync", "mfm_engine_reset", "mfm_engine_get_stats",
    "mfm_engine_stream", "mfm_engine_get_launch_ms", "mfm_engine_get_launch_cycles", "mfm_group_acquire_input", "mfm_group_submit", "mfm_group_shard_engine", "mfm_link_probe", "mfm_link_probe_runs", "mfm_engine_push_pinned_run", "mfm_group_push_pinned_run", "mfm_engine_input_room", "mfm_group_replay_arena", "mfm_strerror", "mfm_last_error", "mfm_hosttwin_discriminate", "mfm_hosttwin_discriminate_batch", "mfm_hosttwin_r14",
    "mfm_hosttwin_pcm_range", "mfm_hosttwin_atan_table", "mfm_hosttwin_atan_table_ok", "mfm_hosttwin_kernel_form",
    "mfm_resampler_create", "mfm_resampler_destroy", "mfm_resampler_max_out", "mfm_resampler_process_device",
    "mfm_resampler_process_host", "mfm_resampler_process_host_to_device",
    "mfm_pocsag_create", "mfm_pocsag_destroy", "mfm_pocsag_process_device", "mfm_pocsag_process_host",
    "mfm_pocsag_fetch_events", "mfm_bch3121_decode_device", "mfm_bch3121_decode_host", "mfm_hosttwin_bch3121_decode",
    "mfm_f32_create", "mfm_f32_add_channel", "mfm_f32_commit", "mfm_f32_destroy", "mfm_f32_max_out",
    "mfm_f32_process_device", "mfm_f32_process_host",
    "mfm_shard_range", "mfm_group_create", "mfm_group_destroy", "mfm_group_add_channel", "mfm_group_commit",
    "mfm_group_nr_shards", "mfm_group_shard_info", "mfm_group_push", "mfm_group_fetch", "mfm_group_release",
    "mfm_group_sync", "mfm_group_get_stats", "mfm_group_exchange_info", "mfm_group_exchange_detail", "mfm_group_rccl_library",
    "mfm_flex_create", "mfm_flex_destroy", "mfm_flex_process_device", "mfm_flex_process_host", "mfm_flex_fetch_events",
    "mfm_mm_create", "mfm_mm_destroy", "mfm_mm_max_decisions", "mfm_mm_process_device", "mfm_mm_process_host",
    "mfm_ais_create", "mfm_ais_destroy", "mfm_ais_process_device", "mfm_ais_process_host", "mfm_ais_fetch_events",
    "mfm_resampler_process_bits_device", "mfm_resampler_process_bits_host_to_device", "mfm_resampler_process_bits_host",
    "mfm_pocsag_process_bits_device", "mfm_ais_process_bits_device", "mfm_hosttwin_splice_bits",
    "mfm_level_create", "mfm_level_destroy", "mfm_level_process_device", "mfm_level_process_host", "mfm_level_fetch",
    "mfm_level_device_view", "mfm_hosttwin_level_window", "mfm_hosttwin_squelch_step",
    "mfm_gate_create", "mfm_gate_destroy", "mfm_gate_process_device", "mfm_gate_process_host", "mfm_gate_fetch",
    "mfm_gate_device_view", "mfm_hosttwin_gate_call",
    "mfm_gate_set_preroll", "mfm_gate_flush_device", "mfm_hosttwin_gate_call_preroll",
    "mfm_resampler_get_form", "mfm_hosttwin_resampler_form", "mfm_hosttwin_resampler_matrix_block",
    "mfm_runrs_create", "mfm_runrs_destroy", "mfm_runrs_process_device", "mfm_runrs_fetch", "mfm_runrs_device_view",
    "mfm_hosttwin_runrs_plan", "mfm_hosttwin_runrs_call",
    "mfm_runrs_get_capacity", "mfm_runais_create", "mfm_runais_destroy", "mfm_runais_process_device", "mfm_runais_fetch",
    "mfm_runais_device_view", "mfm_hosttwin_runais_call",
    "mfm_runpocsag_create", "mfm_runpocsag_destroy", "mfm_runpocsag_process_device", "mfm_runpocsag_fetch", "mfm_runpocsag_device_view",
    "mfm_runpocsag_fetch_state", "mfm_hosttwin_runpocsag_call",
    "mfm_runflex_create", "mfm_runflex_destroy", "mfm_runflex_process_device", "mfm_runflex_fetch", "mfm_runflex_device_view",
    "mfm_runflex_fetch_state", "mfm_hosttwin_runflex_call",
    "mfm_runrs_process_bits_device", "mfm_runrs_bits_view", "mfm_runrs_fetch_bits", "mfm_runrs_get_bits_capacity",
    "mfm_runais_process_bits_device", "mfm_runpocsag_process_bits_device",
    "mfm_hosttwin_runrs_call_bits", "mfm_hosttwin_runais_call_bits", "mfm_hosttwin_runpocsag_call_bits",
    "mfm_pocsag_seek", "mfm_flex_seek", "mfm_ais_seek", "mfm_level_seek", "mfm_gate_seek",
    "mfm_runrs_set_dc_block", "mfm_runrs_get_dc_block", "mfm_hosttwin_runrs_dc_call",
    "mfm_level_set_adaptive", "mfm_level_get_adaptive", "mfm_level_fetch_floor", "mfm_level_floor_view", "mfm_hosttwin_level_adaptive",
    "mfm_runrs_fetch_state", "mfm_runrs_store_state", "mfm_runais_fetch_state", "mfm_runais_store_state",
    "mfm_runpocsag_store_state", "mfm_runflex_store_state",
    "mfm_hosttwin_runrs_state_check", "mfm_hosttwin_runais_state_check", "mfm_hosttwin_runpocsag_state_check",
    "mfm_hosttwin_runflex_state_check",
    "mfm_runais_set_end_report", "mfm_runais_end_stretches_device", "mfm_runais_fetch_ends", "mfm_runais_ends_view",
    "mfm_runpocsag_set_end_report", "mfm_runpocsag_end_stretches_device", "mfm_runpocsag_fetch_ends", "mfm_runpocsag_ends_view",
    "mfm_runflex_set_end_report", "mfm_runflex_end_stretches_device", "mfm_runflex_fetch_ends", "mfm_runflex_ends_view",
    "mfm_hosttwin_runais_call_ends", "mfm_hosttwin_runpocsag_call_ends", "mfm_hosttwin_runflex_call_ends",
    "mfm_hosttwin_runais_end_stretches", "mfm_hosttwin_runpocsag_end_stretches", "mfm_hosttwin_runflex_end_stretches",
    "mfm_runroute_create", "mfm_runroute_destroy", "mfm_runroute_process_device", "mfm_runroute_device_view", "mfm_runroute_fetch",
    "mfm_runroute_get_capacity", "mfm_hosttwin_runroute_capacity", "mfm_hosttwin_runroute_call",
    "mfm_runroute_create_sets", "mfm_runroute_route_channels", "mfm_runroute_route_caps", "mfm_runroute_fetch_payload",
    "mfm_hosttwin_runroute_route_caps", "mfm_hosttwin_runroute_sets_call",
    "mfm_runroute_create_local", "mfm_runroute_bound_view", "mfm_hosttwin_runroute_local_call",
    "mfm_runrs_process_view_device", "mfm_runrs_process_bits_view_device",
    "mfm_runmm_create", "mfm_runmm_destroy", "mfm_runmm_process_device", "mfm_runmm_fetch", "mfm_runmm_device_view",
    "mfm_runmm_fetch_state", "mfm_runmm_store_state", "mfm_hosttwin_runmm_call", "mfm_hosttwin_runmm_state_check",
    "mfm_runmm_get_capacity",
    "mfm_runsync_create", "mfm_runsync_destroy", "mfm_runsync_process_device", "mfm_runsync_fetch", "mfm_runsync_device_view",
    "mfm_runsync_get_capacity", "mfm_runsync_fetch_state", "mfm_runsync_store_state", "mfm_hosttwin_runsync_call",
    "mfm_hosttwin_runsync_state_check",
    "mfm_runbatch_create", "mfm_runbatch_destroy", "mfm_runbatch_process_device", "mfm_runbatch_fetch", "mfm_runbatch_device_view",
    "mfm_runbatch_get_capacity", "mfm_runbatch_fetch_state", "mfm_runbatch_store_state", "mfm_hosttwin_runbatch_call",
    "mfm_hosttwin_runbatch_state_check",
]

class ExchangeDetail(C.Structure):
    """struct mfm_exchange_detail"""
    _fields_ = [("device", C.c_int32), ("rccl_ranks", C.c_int32), ("pci_bus_id", C.c_char * 32), ("timed_exchanges", C.c_uint64),
                ("exchange_ms", C.c_double), ("timed_launches", C.c_uint64), ("kernel_ms", C.c_double), ("bound", C.c_uint32),
                ("reserved0", C.c_uint32)]


def rccl_library():
    """the RCCL file a device group of more than one GPU would use (mfm_group_rccl_library); raises MfmError when none loads"""
    lib = load_library()
    buf = C.create_string_buffer(1024)
    rc = lib.mfm_group_rccl_library(buf, len(buf))
    if rc < 0:
        raise MfmError(rc, "mfm_group_rccl_library", lib.mfm_last_error().decode())
    return buf.value.decode()


MFM_POCSAG_EV_SYNC_FOUND, MFM_POCSAG_EV_BATCH, MFM_POCSAG_EV_SYNC_LOST, MFM_POCSAG_EV_SYNC_KEPT = 1, 2, 3, 4


class MfmError(RuntimeError):
    def __init__(self, code, what, detail):
        super().__init__(f"{what}: {detail} (code {code})")
        self.code = code


class EngineConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("sample_rate_hz", C.c_uint32),
                ("decimation", C.c_uint32), ("max_block_samples", C.c_uint32), ("flags", C.c_uint32),
                ("ext_input", C.c_void_p * 3), ("coalesce_samples", C.c_uint32), ("reserved", C.c_uint32)]


class GroupConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("nr_devices", C.c_uint32), ("devices", C.c_int32 * 16),
                ("sample_rate_hz", C.c_uint32), ("decimation", C.c_uint32), ("max_block_samples", C.c_uint32),
                ("flags", C.c_uint32), ("exchange", C.c_uint32), ("coalesce_samples", C.c_uint32),
                ("reserved", C.c_uint32)]


MFM_X_AUTO, MFM_X_RCCL, MFM_X_RCCL_ALLGATHER = 0, 1, 2


class Block(C.Structure):
    _fields_ = [("first_output", C.c_uint64), ("nr_outputs", C.c_size_t), ("stride", C.c_size_t),
                ("pcm", C.POINTER(C.c_int16)), ("iq", C.POINTER(C.c_int16))]


class Stats(C.Structure):
    _fields_ = [("samples_in", C.c_uint64), ("outputs", C.c_uint64), ("launches", C.c_uint64),
                ("kernel_ms", C.c_double), ("nr_channels", C.c_uint32), ("nr_taps", C.c_uint32),
                ("outputs_per_tile", C.c_uint32), ("lds_bytes", C.c_uint32), ("grid_last", C.c_uint32),
                ("tail_samples", C.c_uint32), ("rot_table_entries", C.c_uint64),
                ("kernel_variant", C.c_uint32), ("pending_blocks", C.c_uint32),
                ("launches_8bit", C.c_uint64), ("timed_launches", C.c_uint64),
                ("rot_exact_channels", C.c_uint32), ("rot_fast_slices", C.c_uint32),
                ("k_steps", C.c_uint32), ("tap_hi_mask", C.c_uint32),
                ("taps_resident", C.c_uint32), ("slice_channels", C.c_uint32),
                ("submits", C.c_uint64), ("pending_samples", C.c_uint64),
                ("overlapped_launches", C.c_uint64), ("pinned", C.c_uint32), ("reserved2", C.c_uint32)]


class PocsagConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("max_events", C.c_uint32), ("flags", C.c_uint32)]


class PocsagEvent(C.Structure):
    _fields_ = [("type", C.c_uint32), ("baud", C.c_uint32), ("channel", C.c_uint32), ("aux", C.c_uint32),
                ("sample", C.c_uint64), ("nr_ok", C.c_uint32), ("fail_mask", C.c_uint32),
                ("raw", C.c_uint32 * 16), ("corrected", C.c_uint32 * 16)]


# numpy view of struct mfm_pocsag_event (160 bytes)
POCSAG_EVENT_DTYPE = np.dtype([("type", "<u4"), ("baud", "<u4"), ("channel", "<u4"), ("aux", "<u4"), ("sample", "<u8"),
                               ("nr_ok", "<u4"), ("fail_mask", "<u4"), ("raw", "<u4", (16,)), ("corrected", "<u4", (16,))])


class AisConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("max_events", C.c_uint32), ("flags", C.c_uint32)]


class AisEvent(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("fcs_valid", C.c_uint32), ("nr_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("sample", C.c_uint64), ("start_sample", C.c_uint64), ("bytes", C.c_uint8 * 160)]


# numpy view of struct mfm_ais_event (192 bytes)
AIS_EVENT_DTYPE = np.dtype([("channel", "<u4"), ("fcs_valid", "<u4"), ("nr_bytes", "<u4"), ("reserved", "<u4"),
                            ("sample", "<u8"), ("start_sample", "<u8"), ("bytes", "u1", (160,))])


class LevelConfig(C.Structure):
    """struct mfm_level_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("form", C.c_uint32), ("window_samples", C.c_uint32),
                ("metric", C.c_uint32), ("sense", C.c_uint32), ("open_thr", C.c_uint64), ("close_thr", C.c_uint64),
                ("hang_windows", C.c_uint32), ("flags", C.c_uint32)]


class LevelAdaptive(C.Structure):
    """struct mfm_level_adaptive"""
    _fields_ = [("floor_windows", C.c_uint32), ("open_q8", C.c_uint32), ("close_q8", C.c_uint32), ("warmup_windows", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class LevelRecord(C.Structure):
    _fields_ = [("energy", C.c_uint64), ("diff_energy", C.c_uint64), ("window", C.c_uint64), ("peak", C.c_uint32),
                ("channel", C.c_uint32), ("open", C.c_uint32), ("reserved", C.c_uint32)]


# numpy view of struct mfm_level_record (40 bytes)
LEVEL_RECORD_DTYPE = np.dtype([("energy", "<u8"), ("diff_energy", "<u8"), ("window", "<u8"), ("peak", "<u4"),
                               ("channel", "<u4"), ("open", "<u4"), ("reserved", "<u4")])
MFM_LEVEL_PCM, MFM_LEVEL_IQ = 0, 1
MFM_LEVEL_METRIC_ENERGY, MFM_LEVEL_METRIC_DIFF = 0, 1
MFM_LEVEL_OPEN_ABOVE, MFM_LEVEL_OPEN_BELOW = 0, 1


class GateConfig(C.Structure):
    """struct mfm_gate_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("window_samples", C.c_uint32), ("elems_per_sample", C.c_uint32),
                ("max_open_windows", C.c_uint32), ("flags", C.c_uint32)]


class GateRun(C.Structure):
    _fields_ = [("first_window", C.c_uint64), ("payload_offset", C.c_uint64), ("channel", C.c_uint32), ("nr_windows", C.c_uint32)]


MFM_GATE_MAX_PREROLL = 63               # pre-roll windows at most
MFM_GATE_MAX_HISTORY_BYTES = 1 << 30    # one history buffer of a gate with pre-roll at most
# numpy view of struct mfm_gate_run (24 bytes)
GATE_RUN_DTYPE = np.dtype([("first_window", "<u8"), ("payload_offset", "<u8"), ("channel", "<u4"), ("nr_windows", "<u4")])


class RunrsConfig(C.Structure):
    """struct mfm_runrs_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("interpolate", C.c_uint32),
                ("decimate", C.c_uint32), ("window_samples", C.c_uint32), ("max_windows", C.c_uint32), ("max_runs", C.c_uint32),
                ("invert", C.c_uint32), ("flags", C.c_uint32), ("max_in_samples", C.c_uint32), ("preroll_windows", C.c_uint32)]


class RunrsRun(C.Structure):
    _fields_ = [("first_window", C.c_uint64), ("out_offset", C.c_uint64), ("first_out", C.c_uint64), ("channel", C.c_uint32),
                ("nr_out", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


MFM_RUNRS_MAX_LDS_BYTES = 49152
MFM_RUNRS_BEGINS = 1                                    # mfm_runrs_run.flags bit 0: the run begins a stretch
MFM_RUNRS_OVER_OWN, MFM_RUNRS_OVER_GATE = 1, 2          # d_totals[2]
MFM_RUNRS_GATE_OUT_OF_STEP, MFM_RUNRS_GATE_BAD_RUNS = 1, 2  # d_totals[3]
MFM_RUNRS_NO_WINDOW = (1 << 64) - 1                     # mfm_runrs_state.expected of a channel without a stretch
# numpy views of struct mfm_runrs_run (40 bytes) and struct mfm_runrs_state (24 bytes, the host twin's per-channel state)
RUNRS_RUN_DTYPE = np.dtype([("first_window", "<u8"), ("out_offset", "<u8"), ("first_out", "<u8"), ("channel", "<u4"),
                            ("nr_out", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
RUNRS_STATE_DTYPE = np.dtype([("expected", "<u8"), ("outs", "<u8"), ("phase", "<u4"), ("pending", "<u4")])
# struct mfm_runrs_dc_state (16 bytes): the per-channel state of the burst resampler's DC blocker, all zero at the start of a stream
RUNRS_DC_STATE_DTYPE = np.dtype([("x_n_1", "<i4"), ("y_n_1", "<i4"), ("acc", "<i4"), ("reserved", "<u4")])


class RunrsBitsView(C.Structure):
    """struct mfm_runrs_bits_view: the burst resampler's bits form, valid until its next process call of either form"""
    _fields_ = [("d_runs", C.c_void_p), ("d_bits", C.c_void_p), ("d_totals", C.c_void_p), ("polarity", C.c_uint32),
                ("reserved", C.c_uint32)]


class RunRouteConfig(C.Structure):
    """struct mfm_runroute_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("nr_routes", C.c_uint32),
                ("window_samples", C.c_uint32), ("max_windows", C.c_uint32), ("max_runs", C.c_uint32), ("max_in_samples", C.c_uint32),
                ("preroll_windows", C.c_uint32), ("flags", C.c_uint32)]


MFM_RUNROUTE_MAX_ROUTES = 8
MFM_ROUTE_NONE = 255    # a channel whose runs go to no route
MFM_RUNROUTE_F_PACK = 1  # mfm_runroute_create_sets: route-local channels and a dense payload per route


class RunaisConfig(C.Structure):
    """struct mfm_runais_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_out_samples", C.c_uint32), ("max_events", C.c_uint32), ("flags", C.c_uint32)]


class RunaisEvent(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("fcs_valid", C.c_uint32), ("nr_bytes", C.c_uint32), ("run", C.c_uint32),
                ("stretch_window", C.c_uint64), ("sample", C.c_uint64), ("start_sample", C.c_uint64), ("bytes", C.c_uint8 * 160)]


MFM_RUNAIS_OVER_RUNS, MFM_RUNAIS_OVER_EVENTS = 1, 2                                # d_totals[2]
MFM_RUNAIS_IN_RUNRS, MFM_RUNAIS_IN_OUT_OF_STEP, MFM_RUNAIS_IN_BAD_RUNS = 1, 2, 4   # d_totals[3]
# numpy views of struct mfm_runais_event (200 bytes) and struct mfm_runais_state (264 bytes, per channel)
RUNAIS_EVENT_DTYPE = np.dtype([("channel", "<u4"), ("fcs_valid", "<u4"), ("nr_bytes", "<u4"), ("run", "<u4"),
                               ("stretch_window", "<u8"), ("sample", "<u8"), ("start_sample", "<u8"), ("bytes", "u1", (160,))])
RUNAIS_STATE_DTYPE = np.dtype([("outs", "<u8"), ("stretch_window", "<u8"), ("pos", "<u8"), ("r", "<u8"), ("rd", "<u8"),
                               ("start", "<u8"), ("mode", "<u4"), ("last_sample", "<u4"), ("hist8", "<u4"), ("cur_bit", "<u4"),
                               ("has_stretch", "<u4"), ("reserved", "<u4"), ("packet", "<u4", (40,)), ("tail", "<u4", (8,))])


class RunPocsagConfig(C.Structure):
    """struct mfm_runpocsag_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_out_samples", C.c_uint32), ("max_events", C.c_uint32), ("flags", C.c_uint32)]


class RunPocsagEvent(C.Structure):
    _fields_ = [("type", C.c_uint32), ("baud", C.c_uint32), ("channel", C.c_uint32), ("aux", C.c_uint32), ("run", C.c_uint32),
                ("nr_ok", C.c_uint32), ("fail_mask", C.c_uint32), ("reserved", C.c_uint32), ("stretch_window", C.c_uint64),
                ("sample", C.c_uint64), ("raw", C.c_uint32 * 16), ("corrected", C.c_uint32 * 16)]


MFM_RUNPOCSAG_OVER_RUNS, MFM_RUNPOCSAG_OVER_EVENTS = 1, 2                                   # d_totals[2]
MFM_RUNPOCSAG_IN_RUNRS, MFM_RUNPOCSAG_IN_OUT_OF_STEP, MFM_RUNPOCSAG_IN_BAD_RUNS = 1, 2, 4   # d_totals[3]
RUNPOCSAG_MIN_SPACING = 544 * 16   # samples between two BATCH events of a stretch at least (csrc/mfm_runpocsag.h)
# numpy views of struct mfm_runpocsag_event (176 bytes) and struct mfm_runpocsag_state (432 bytes, per channel)
RUNPOCSAG_EVENT_DTYPE = np.dtype([("type", "<u4"), ("baud", "<u4"), ("channel", "<u4"), ("aux", "<u4"), ("run", "<u4"),
                                  ("nr_ok", "<u4"), ("fail_mask", "<u4"), ("reserved", "<u4"), ("stretch_window", "<u8"),
                                  ("sample", "<u8"), ("raw", "<u4", (16,)), ("corrected", "<u4", (16,))])
RUNPOCSAG_STATE_DTYPE = np.dtype([("outs", "<u8"), ("stretch_window", "<u8"), ("mode", "<u4"), ("baud", "<u4"), ("spb", "<u4"),
                                  ("skip", "<u4"), ("batch_word", "<u4"), ("batch_bit", "<u4"), ("sync_word", "<u4"),
                                  ("nr_sync_bits", "<u4"), ("nr_eye", "<u4", (3,)), ("since_reset", "<u4"), ("has_stretch", "<u4"),
                                  ("batch", "<u4", (16,)), ("tail", "<u4", (75,))])


class RunMmConfig(C.Structure):
    """struct mfm_runmm_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_out_samples", C.c_uint32), ("max_decisions", C.c_uint32), ("flags", C.c_uint32), ("kw", C.c_float),
                ("km", C.c_float), ("samples_per_bit", C.c_float), ("error_min", C.c_float), ("error_max", C.c_float)]


MFM_RUNMM_OVER_RUNS, MFM_RUNMM_OVER_DECISIONS = 1, 2                                # d_totals[2]
MFM_RUNMM_IN_RUNRS, MFM_RUNMM_IN_OUT_OF_STEP, MFM_RUNMM_IN_BAD_RUNS = 1, 2, 4       # d_totals[3]
RUNMM_STAGING_UNIT = 512   # samples of a run the walk holds in LDS at a time (csrc/mfm_runmm.h)
# numpy views of struct mfm_runmm_run (40 bytes, per run) and struct mfm_runmm_state (48 bytes, per channel)
RUNMM_RUN_DTYPE = np.dtype([("first_window", "<u8"), ("dec_offset", "<u8"), ("first_dec", "<u8"), ("channel", "<u4"),
                            ("nr_dec", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
RUNMM_STATE_DTYPE = np.dtype([("outs", "<u8"), ("decs", "<u8"), ("stretch_window", "<u8"), ("w", "<f4"), ("m", "<f4"),
                              ("last_sample", "<f4"), ("next_offset", "<u4"), ("has_stretch", "<u4"), ("reserved", "<u4")])


class RunSyncConfig(C.Structure):
    """struct mfm_runsync_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_decisions", C.c_uint32), ("max_events", C.c_uint32), ("nr_words", C.c_uint32), ("words", C.c_uint32 * 8),
                ("max_distance", C.c_uint32), ("bit_rule", C.c_uint32), ("flags", C.c_uint32)]


MFM_RUNSYNC_BIT_NOT_POS, MFM_RUNSYNC_BIT_POS = 0, 1                                 # bit = !(d > 0) / bit = (d > 0)
MFM_RUNSYNC_F_EITHER = 1                                                            # the complement of every word too
MFM_RUNSYNC_OVER_RUNS, MFM_RUNSYNC_OVER_DECISIONS, MFM_RUNSYNC_OVER_EVENTS = 1, 2, 4    # d_totals[2]
MFM_RUNSYNC_IN_RUNMM, MFM_RUNSYNC_IN_OUT_OF_STEP, MFM_RUNSYNC_IN_BAD_RUNS = 1, 2, 4     # d_totals[3]
RUNSYNC_SEGMENT = 1024   # decisions of a run one wave packs and matches (csrc/mfm_runsync.h)
# numpy views of struct mfm_runsync_run (40 bytes, per run), mfm_runsync_event (32 bytes) and mfm_runsync_state (24 bytes, per channel)
RUNSYNC_RUN_DTYPE = np.dtype([("first_window", "<u8"), ("word_offset", "<u8"), ("first_dec", "<u8"), ("channel", "<u4"),
                              ("nr_dec", "<u4"), ("flags", "<u4"), ("nr_events", "<u4")])
RUNSYNC_EVENT_DTYPE = np.dtype([("dec", "<u8"), ("channel", "<u4"), ("run", "<u4"), ("seen", "<u4"), ("word_index", "<u4"),
                                ("distance", "<u4"), ("inverted", "<u4")])
RUNSYNC_STATE_DTYPE = np.dtype([("stretch_window", "<u8"), ("decs", "<u8"), ("shr", "<u4"), ("has_stretch", "<u4")])


class RunBatchConfig(C.Structure):
    """struct mfm_runbatch_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_decisions", C.c_uint32), ("max_events", C.c_uint32), ("nr_words", C.c_uint32), ("words", C.c_uint32 * 8),
                ("word_mask", C.c_uint32), ("keep_distance", C.c_uint32), ("flags", C.c_uint32)]


MFM_RUNBATCH_SEARCH, MFM_RUNBATCH_RECEIVE, MFM_RUNBATCH_SLOT = 0, 1, 2                   # mfm_runbatch_state.mode
MFM_RUNBATCH_OVER_RUNS, MFM_RUNBATCH_OVER_EVENTS = 1, 2                                 # d_totals[2]
MFM_RUNBATCH_IN_RUNSYNC, MFM_RUNBATCH_IN_OUT_OF_STEP, MFM_RUNBATCH_IN_BAD_RUNS, MFM_RUNBATCH_IN_BAD_EVENTS = 1, 2, 4, 8   # d_totals[3]
RUNBATCH_FRAME = 544     # decisions of a batch and the sync slot behind it (csrc/mfm_runbatch.h)
# numpy views of struct mfm_runbatch_event (176 bytes) and mfm_runbatch_state (120 bytes, per channel)
RUNBATCH_EVENT_DTYPE = np.dtype([("type", "<u4"), ("channel", "<u4"), ("run", "<u4"), ("aux", "<u4"), ("word_index", "<u4"),
                                 ("inverted", "<u4"), ("nr_ok", "<u4"), ("fail_mask", "<u4"), ("stretch_window", "<u8"), ("dec", "<u8"),
                                 ("raw", "<u4", (16,)), ("corrected", "<u4", (16,))])
RUNBATCH_STATE_DTYPE = np.dtype([("stretch_window", "<u8"), ("decs", "<u8"), ("mark", "<u8"), ("has_stretch", "<u4"), ("mode", "<u4"),
                                 ("word_index", "<u4"), ("inverted", "<u4"), ("nr_kept", "<u4"), ("reserved", "<u4"),
                                 ("kept", "<u4", (17,)), ("reserved2", "<u4")])


def runmm_min_step(km, error_min):
    """s = floor(error_min - |km| * 32768) in float: no step of the loop is shorter (csrc/mfm_runmm.h)"""
    return int(np.floor(np.float32(error_min) - np.abs(np.float32(km)) * np.float32(32768.0)))


def runmm_slots(nr_out, s):
    """the decision bound of a run of nr_out samples (mfm_runmm_slots)"""
    return int(nr_out) // int(s) + 1


def runpocsag_slots(nr_out):
    """the event bound of a run of nr_out samples (mfm_runpocsag_slots)"""
    return 3 * (int(nr_out) // RUNPOCSAG_MIN_SPACING + 1) + 2


class FlexConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("max_events", C.c_uint32), ("flags", C.c_uint32)]


# numpy views of struct mfm_flex_event (88 bytes) and struct mfm_flex_frame_words
FLEX_EVENT_DTYPE = np.dtype([("type", "<u4"), ("channel", "<u4"), ("sample", "<u8"), ("sync_sample", "<u8"),
                             ("coding", "<u4"), ("baud", "<u4"), ("eye", "<u4"), ("a", "<u4"), ("b", "<u4"),
                             ("inv_a", "<u4"), ("fiw_raw", "<u4"), ("fiw", "<u4"), ("fiw_rc", "<u4"),
                             ("sample_range", "<i4"), ("sample_delta", "<i4"), ("cycle", "<u4"), ("frame", "<u4"),
                             ("frame_index", "<u4"), ("nr_phases", "<u4"), ("reserved", "<u4")])
FLEX_FRAME_DTYPE = np.dtype([("words", "<u4", (4, 88))])
MFM_FLEX_EV_FRAME, MFM_FLEX_EV_BAD_BAUD, MFM_FLEX_EV_BAD_FIW = 1, 2, 3


class RunFlexConfig(C.Structure):
    """struct mfm_runflex_config"""
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32), ("max_runs", C.c_uint32),
                ("max_out_samples", C.c_uint32), ("max_events", C.c_uint32), ("max_frames", C.c_uint32), ("flags", C.c_uint32)]


MFM_RUNFLEX_OVER_RUNS, MFM_RUNFLEX_OVER_EVENTS = 1, 2                                 # d_totals[2]
MFM_RUNFLEX_IN_RUNRS, MFM_RUNFLEX_IN_OUT_OF_STEP, MFM_RUNFLEX_IN_BAD_RUNS = 1, 2, 4   # d_totals[3]
RUNFLEX_EVENT_SPACING = 1105    # samples between two events of a stretch at least (csrc/mfm_runflex.h)
RUNFLEX_FRAME_SPACING = 29985   # samples between two FRAME events of a stretch at least
RUNFLEX_RING = 32768            # PCM samples per channel the stage keeps
# numpy views of struct mfm_runflex_event (104 bytes: mfm_flex_event, then run and stretch) and struct mfm_runflex_state (88
# bytes, per channel)
RUNFLEX_EVENT_DTYPE = np.dtype(FLEX_EVENT_DTYPE.descr + [("run", "<u4"), ("reserved2", "<u4"), ("stretch_window", "<u8")])
RUNFLEX_STATE_DTYPE = np.dtype([("outs", "<u8"), ("stretch_window", "<u8"), ("p", "<u8"), ("j", "<u8"), ("mode", "<u4"),
                                ("run", "<u4"), ("eye", "<u4"), ("coding", "<u4"), ("a", "<u4"), ("b", "<u4"), ("inv_a", "<u4"),
                                ("fiw_raw", "<u4"), ("fiw", "<u4"), ("sample_range", "<i4"), ("sample_delta", "<i4"),
                                ("cycle", "<u4"), ("frame", "<u4"), ("has_stretch", "<u4")])


def runflex_event_bound(nr_out):
    """the event bound of a run of nr_out samples (mfm_runflex_event_slots)"""
    return int(nr_out) // RUNFLEX_EVENT_SPACING + 1


def runflex_frame_bound(nr_out):
    """the frame bound of a run of nr_out samples (mfm_runflex_frame_slots)"""
    return int(nr_out) // RUNFLEX_FRAME_SPACING + 1


class ResamplerConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("interpolate", C.c_uint32), ("decimate", C.c_uint32), ("max_in_samples", C.c_uint32),
                ("invert", C.c_uint32), ("dc_block", C.c_uint32), ("dc_pole", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


MFM_RS_FORCE_DOT2 = 1
# mfm_resampler_form.fallback: why the matrix form was not taken
MFM_RS_FB_NONE, MFM_RS_FB_RATIO, MFM_RS_FB_WINDOW, MFM_RS_FB_BLOCK, MFM_RS_FB_TAP_RANGE, MFM_RS_FB_FORCED = 0, 1, 2, 3, 4, 5


class ResamplerForm(C.Structure):
    """struct mfm_resampler_form: the kernel a resampler runs (form 0 v_dot2, 1 matrix) and its geometry"""
    _fields_ = [("form", C.c_uint32), ("fallback", C.c_uint32), ("reg_pairs", C.c_uint32), ("k_steps", C.c_uint32),
                ("block_samples", C.c_uint32), ("row_bytes", C.c_uint32), ("window_bytes", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("phase_len", C.c_uint32), ("max_out", C.c_uint32), ("dc_p", C.c_int32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class BitsView(C.Structure):
    """struct mfm_bits_view: one packed predicate bit per resampler output, in device memory, valid until the resampler's
    next process call.  Output j of the call is bit j % 32 of word j / 32 of its channel's row."""
    _fields_ = [("d_bits", C.c_void_p), ("stride_words", C.c_size_t), ("nr_bits", C.c_size_t), ("polarity", C.c_uint32),
                ("reserved", C.c_uint32)]


class F32Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("sample_rate_hz", C.c_uint32),
                ("decimation", C.c_uint32), ("max_block_samples", C.c_uint32), ("flags", C.c_uint32)]


class F32Block(C.Structure):
    _fields_ = [("d_pcm_f32", C.c_void_p), ("d_pcm_i16", C.c_void_p), ("d_iq_f32", C.c_void_p),
                ("stride", C.c_size_t), ("nr_out", C.c_size_t), ("nr_channels", C.c_uint32), ("reserved", C.c_uint32)]


MFM_F32_WANT_IQ = 1
MFM_F32_PACKED_FMA = 2
MFM_F32_TILE_KERNEL = 4


class MmConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("nr_channels", C.c_uint32),
                ("max_in_samples", C.c_uint32), ("kw", C.c_float), ("km", C.c_float), ("samples_per_bit", C.c_float),
                ("error_min", C.c_float), ("error_max", C.c_float)]

_lib = None


def load_library():
    """dlopen libmultifm_hip.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make -C tsl-sdr_amd` (hipcc, gfx950). "
                          "There is no CPU fallback for the multifm engine.")
    lib = C.CDLL(LIB_PATH)
    vp, i16p = C.c_void_p, C.POINTER(C.c_int16)
    lib.mfm_engine_input_bytes.restype = C.c_size_t
    lib.mfm_engine_input_bytes.argtypes = [C.c_uint32, C.c_uint32]
    lib.mfm_engine_input_bytes_cfg.restype = C.c_size_t
    lib.mfm_engine_input_bytes_cfg.argtypes = [C.POINTER(EngineConfig), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mfm_engine_flush.argtypes = [vp]
    lib.mfm_engine_replay.argtypes = [vp, C.c_size_t, C.c_size_t]
    lib.mfm_engine_seek.argtypes = [vp, C.c_uint64]
    for name in ("mfm_pocsag_seek", "mfm_flex_seek", "mfm_ais_seek", "mfm_level_seek", "mfm_gate_seek"):
        getattr(lib, name).argtypes = [vp, C.c_uint64]
    lib.mfm_host_alloc.argtypes = [C.c_size_t]
    lib.mfm_host_alloc.restype = vp
    lib.mfm_host_free.argtypes = [vp]
    lib.mfm_host_free.restype = None
    lib.mfm_engine_push_pinned.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    lib.mfm_engine_copy_done.argtypes = [vp, C.c_uint64]
    lib.mfm_engine_copy_wait.argtypes = [vp, C.c_uint64]
    lib.mfm_group_push_pinned.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    lib.mfm_group_copy_done.argtypes = [vp, C.c_uint64]
    lib.mfm_group_replay_pinned.argtypes = [vp, C.POINTER(vp), C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_uint64)]
    lib.mfm_group_copy_wait.argtypes = [vp, C.c_uint64]
    lib.mfm_engine_last_launch_input.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    lib.mfm_group_flush.argtypes = [vp]
    lib.mfm_engine_create.argtypes = [C.POINTER(vp), C.POINTER(EngineConfig)]
    lib.mfm_engine_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_engine_destroy.restype = None
    lib.mfm_engine_add_channel.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_int]
    lib.mfm_engine_add_channel_q14.argtypes = [vp, i16p, i16p, C.c_size_t, C.c_int16, C.c_int16, C.c_int]
    lib.mfm_engine_get_channel.argtypes = [vp, C.c_uint32, i16p, i16p, i16p]
    lib.mfm_engine_commit.argtypes = [vp]
    lib.mfm_engine_acquire_input.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.mfm_engine_acquire_input_bytes.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.mfm_engine_submit.argtypes = [vp, C.c_size_t, vp, C.c_int]
    lib.mfm_engine_push.argtypes = [vp, i16p, C.c_size_t]
    lib.mfm_engine_push_bytes.argtypes = [vp, vp, C.c_size_t, C.c_int]
    lib.mfm_engine_fetch.argtypes = [vp, C.POINTER(Block)]
    lib.mfm_engine_release.argtypes = [vp]
    lib.mfm_engine_last_output_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_size_t), C.POINTER(vp)]
    lib.mfm_engine_sync.argtypes = [vp]
    lib.mfm_engine_reset.argtypes = [vp]
    lib.mfm_engine_get_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.mfm_engine_stream.argtypes = [vp]
    lib.mfm_shard_range.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.mfm_shard_range.restype = None
    lib.mfm_group_create.argtypes = [C.POINTER(vp), C.POINTER(GroupConfig)]
    lib.mfm_group_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_group_destroy.restype = None
    lib.mfm_group_add_channel.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_int]
    lib.mfm_group_commit.argtypes = [vp]
    lib.mfm_group_nr_shards.argtypes = [vp]
    lib.mfm_group_shard_info.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    lib.mfm_group_push.argtypes = [vp, vp, C.c_size_t, C.c_int]
    lib.mfm_group_fetch.argtypes = [vp, C.POINTER(Block)]
    lib.mfm_group_release.argtypes = [vp]
    lib.mfm_group_sync.argtypes = [vp]
    lib.mfm_group_get_stats.argtypes = [vp, C.c_uint32, C.POINTER(Stats)]
    lib.mfm_group_exchange_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mfm_group_acquire_input.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.mfm_group_submit.argtypes = [vp, C.c_size_t]
    lib.mfm_group_shard_engine.argtypes = [vp, C.c_uint32]
    lib.mfm_group_shard_engine.restype = vp
    lib.mfm_link_probe.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mfm_engine_push_pinned_run.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    lib.mfm_group_push_pinned_run.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    lib.mfm_engine_input_room.argtypes = [vp]
    lib.mfm_engine_input_room.restype = C.c_size_t
    lib.mfm_group_replay_arena.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]
    lib.mfm_link_probe_runs.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]
    lib.mfm_engine_get_launch_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
    lib.mfm_engine_get_launch_ms.restype = C.c_size_t
    lib.mfm_engine_get_launch_cycles.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t]
    lib.mfm_engine_get_launch_cycles.restype = C.c_size_t
    lib.mfm_engine_stream.restype = vp
    if hasattr(lib, "mfm_group_exchange_detail"):   # (an older library under MFM_LIB, tools/exp/ab.py: same-box A/B against it)
        lib.mfm_group_exchange_detail.argtypes = [vp, C.c_uint32, vp]
        lib.mfm_group_rccl_library.argtypes = [C.c_char_p, C.c_size_t]
    lib.mfm_strerror.argtypes = [C.c_int]
    lib.mfm_strerror.restype = C.c_char_p
    lib.mfm_last_error.restype = C.c_char_p
    lib.mfm_hosttwin_discriminate.argtypes = [C.c_int32, C.c_int32]
    lib.mfm_hosttwin_discriminate.restype = C.c_int32
    lib.mfm_hosttwin_discriminate_batch.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, i16p]
    lib.mfm_hosttwin_discriminate_batch.restype = None
    lib.mfm_devtest_discriminate.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, i16p, C.c_int]
    lib.mfm_devtest_rcp_table.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mfm_hosttwin_r14.argtypes = [C.c_int32]
    lib.mfm_hosttwin_r14.restype = C.c_int16
    lib.mfm_hosttwin_pcm_range.argtypes = [C.c_uint32, C.c_uint32, i16p]
    lib.mfm_hosttwin_pcm_range.restype = None
    lib.mfm_hosttwin_atan_table.argtypes = [C.POINTER(C.c_float)]
    lib.mfm_hosttwin_atan_table.restype = None
    lib.mfm_hosttwin_atan_table_ok.restype = C.c_int
    lib.mfm_hosttwin_kernel_form.argtypes = [vp, C.POINTER(Stats)]
    u32p = C.POINTER(C.c_uint32)
    lib.mfm_pocsag_create.argtypes = [C.POINTER(vp), C.POINTER(PocsagConfig)]
    lib.mfm_pocsag_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_pocsag_destroy.restype = None
    lib.mfm_pocsag_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.mfm_pocsag_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t]
    lib.mfm_pocsag_fetch_events.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_ais_create.argtypes = [C.POINTER(vp), C.POINTER(AisConfig)]
    lib.mfm_ais_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_ais_destroy.restype = None
    lib.mfm_ais_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.mfm_ais_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t]
    lib.mfm_ais_fetch_events.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_flex_create.argtypes = [C.POINTER(vp), C.POINTER(FlexConfig)]
    lib.mfm_flex_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_flex_destroy.restype = None
    lib.mfm_flex_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.mfm_flex_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t]
    lib.mfm_flex_fetch_events.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_bch3121_decode_device.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    lib.mfm_bch3121_decode_host.argtypes = [u32p, C.POINTER(C.c_uint8), C.c_size_t, C.c_int]
    lib.mfm_hosttwin_bch3121_decode.argtypes = [u32p]
    lib.mfm_resampler_create.argtypes = [C.POINTER(vp), C.POINTER(ResamplerConfig), i16p, C.c_size_t]
    lib.mfm_resampler_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_resampler_destroy.restype = None
    lib.mfm_resampler_max_out.argtypes = [vp]
    lib.mfm_resampler_max_out.restype = C.c_size_t
    lib.mfm_resampler_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(vp),
                                                 C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.mfm_resampler_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, i16p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_resampler_process_host_to_device.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, vp, C.POINTER(vp),
                                                         C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    if hasattr(lib, "mfm_resampler_process_bits_device"):   # (an older library under MFM_LIB)
        lib.mfm_resampler_process_bits_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_uint32, C.POINTER(BitsView)]
        lib.mfm_resampler_process_bits_host_to_device.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, vp, C.c_uint32, C.POINTER(BitsView)]
        lib.mfm_resampler_process_bits_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, C.c_uint32, u32p, C.c_size_t,
                                                        C.POINTER(C.c_size_t)]
        lib.mfm_pocsag_process_bits_device.argtypes = [vp, C.POINTER(BitsView), vp]
        lib.mfm_ais_process_bits_device.argtypes = [vp, C.POINTER(BitsView), vp]
        lib.mfm_hosttwin_splice_bits.argtypes = [u32p, C.c_uint64, u32p, C.c_uint64]
        lib.mfm_hosttwin_splice_bits.restype = None
    u64p = C.POINTER(C.c_uint64)
    lib.mfm_level_create.argtypes = [C.POINTER(vp), C.POINTER(LevelConfig)]
    lib.mfm_level_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_level_destroy.restype = None
    lib.mfm_level_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.mfm_level_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t]
    lib.mfm_level_fetch.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_level_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(vp)]
    lib.mfm_hosttwin_level_window.argtypes = [i16p, C.c_size_t, C.c_uint32, C.c_int16, u64p, u64p, u32p]
    lib.mfm_hosttwin_level_window.restype = None
    lib.mfm_hosttwin_squelch_step.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, u32p, u32p]
    lib.mfm_hosttwin_squelch_step.restype = C.c_uint32
    lib.mfm_level_set_adaptive.argtypes = [vp, C.POINTER(LevelAdaptive)]
    lib.mfm_level_get_adaptive.argtypes = [vp, u32p, C.POINTER(LevelAdaptive)]
    lib.mfm_level_fetch_floor.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_level_floor_view.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.mfm_hosttwin_level_adaptive.argtypes = [u64p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(LevelAdaptive),
                                                u64p, u32p]
    lib.mfm_hosttwin_level_adaptive.restype = None
    szp = C.POINTER(C.c_size_t)
    lib.mfm_gate_create.argtypes = [C.POINTER(vp), C.POINTER(GateConfig)]
    lib.mfm_gate_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_gate_destroy.restype = None
    lib.mfm_gate_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp]
    lib.mfm_gate_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t]
    lib.mfm_gate_fetch.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_gate_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_gate_set_preroll.argtypes = [vp, C.c_uint32]
    lib.mfm_gate_flush_device.argtypes = [vp, vp]
    lib.mfm_hosttwin_gate_call_preroll.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, i16p, C.c_size_t,
                                                   C.c_size_t, i16p, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_hosttwin_gate_call.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, i16p, C.c_size_t, C.c_size_t, i16p, vp,
                                           C.c_size_t, C.c_size_t, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runrs_create.argtypes = [C.POINTER(vp), C.POINTER(RunrsConfig), i16p, C.c_size_t]
    lib.mfm_runrs_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runrs_destroy.restype = None
    lib.mfm_runrs_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runrs_fetch.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runrs_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runrs_get_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.mfm_runrs_process_bits_device.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    lib.mfm_runrs_process_view_device.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mfm_runrs_process_bits_view_device.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp]
    lib.mfm_runrs_bits_view.argtypes = [vp, C.POINTER(RunrsBitsView)]
    lib.mfm_runrs_fetch_bits.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runrs_get_bits_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.mfm_runrs_set_dc_block.argtypes = [vp, C.c_uint32, C.c_double]
    lib.mfm_runrs_get_dc_block.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    lib.mfm_hosttwin_runrs_dc_call.argtypes = [C.c_uint32, C.c_double, vp, vp, C.c_size_t, vp, C.c_size_t]
    lib.mfm_runais_process_bits_device.argtypes = [vp, C.POINTER(RunrsBitsView), vp]
    lib.mfm_runpocsag_process_bits_device.argtypes = [vp, C.POINTER(RunrsBitsView), vp]
    lib.mfm_hosttwin_runrs_call_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, i16p, C.c_size_t, vp,
                                                 i16p, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_hosttwin_runais_call_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t,
                                                  szp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runpocsag_call_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp,
                                                     C.c_size_t, szp, C.POINTER(C.c_uint32)]
    lib.mfm_runais_create.argtypes = [C.POINTER(vp), C.POINTER(RunaisConfig)]
    lib.mfm_runais_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runais_destroy.restype = None
    lib.mfm_runais_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runais_fetch.argtypes = [vp, vp, C.c_size_t, szp]
    lib.mfm_runais_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runpocsag_create.argtypes = [C.POINTER(vp), C.POINTER(RunPocsagConfig)]
    lib.mfm_runpocsag_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runpocsag_destroy.restype = None
    lib.mfm_runpocsag_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runpocsag_fetch.argtypes = [vp, vp, C.c_size_t, szp]
    lib.mfm_runpocsag_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runpocsag_fetch_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runflex_create.argtypes = [C.POINTER(vp), C.POINTER(RunFlexConfig)]
    lib.mfm_runflex_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runflex_destroy.restype = None
    lib.mfm_runflex_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runflex_fetch.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runflex_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runflex_fetch_state.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mfm_runrs_fetch_state.argtypes = [vp, vp, vp, vp, C.c_size_t]
    lib.mfm_runrs_store_state.argtypes = [vp, vp, vp, vp, C.c_size_t]
    lib.mfm_runais_fetch_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runais_store_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runpocsag_store_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runflex_store_state.argtypes = [vp, vp, vp, C.c_size_t]
    lib.mfm_hosttwin_runrs_state_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    lib.mfm_hosttwin_runais_state_check.argtypes = [C.c_uint32, vp]
    lib.mfm_hosttwin_runpocsag_state_check.argtypes = [C.c_uint32, vp]
    lib.mfm_hosttwin_runflex_state_check.argtypes = [C.c_uint32, vp]
    for st in ("runais", "runpocsag", "runflex"):
        getattr(lib, f"mfm_{st}_set_end_report").argtypes = [vp, C.c_int]
        getattr(lib, f"mfm_{st}_end_stretches_device").argtypes = [vp, vp]
        getattr(lib, f"mfm_{st}_fetch_ends").argtypes = [vp, vp, C.c_size_t, szp]
        getattr(lib, f"mfm_{st}_ends_view").argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        getattr(lib, f"mfm_hosttwin_{st}_end_stretches").argtypes = [C.c_uint32, vp, vp, C.c_size_t, szp]
    lib.mfm_hosttwin_runais_call_ends.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_size_t, szp,
                                                  C.POINTER(C.c_uint32), vp, C.c_size_t, szp]
    lib.mfm_hosttwin_runpocsag_call_ends.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_size_t, szp,
                                                     C.POINTER(C.c_uint32), vp, C.c_size_t, szp]
    lib.mfm_hosttwin_runflex_call_ends.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                                   C.c_size_t, szp, vp, C.c_size_t, szp, C.POINTER(C.c_uint32), vp, C.c_size_t, szp]
    lib.mfm_runroute_create.argtypes = [C.POINTER(vp), C.POINTER(RunRouteConfig), vp]
    lib.mfm_runroute_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runroute_destroy.restype = None
    lib.mfm_runroute_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runroute_device_view.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runroute_fetch.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp, szp]
    lib.mfm_runroute_get_capacity.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runroute_capacity.argtypes = [C.POINTER(RunRouteConfig), vp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runroute_call.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp]
    u32p = C.POINTER(C.c_uint32)
    lib.mfm_runroute_create_sets.argtypes = [C.POINTER(vp), C.POINTER(RunRouteConfig), vp]
    lib.mfm_runroute_route_channels.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.mfm_runroute_route_caps.argtypes = [vp, C.c_uint32, u32p, u32p, u32p]
    lib.mfm_runroute_fetch_payload.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.mfm_hosttwin_runroute_route_caps.argtypes = [C.POINTER(RunRouteConfig), vp, C.c_uint32, u32p, u32p, u32p]
    lib.mfm_hosttwin_runroute_sets_call.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, vp, vp,
                                                    vp, C.c_size_t]
    lib.mfm_runroute_create_local.argtypes = [C.POINTER(vp), C.POINTER(RunRouteConfig), vp]
    lib.mfm_runroute_bound_view.argtypes = [vp, C.POINTER(vp)]
    lib.mfm_hosttwin_runroute_local_call.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    lib.mfm_runmm_create.argtypes = [C.POINTER(vp), C.POINTER(RunMmConfig)]
    lib.mfm_runmm_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runmm_destroy.restype = None
    lib.mfm_runmm_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runmm_fetch.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runmm_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runmm_fetch_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runmm_store_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_hosttwin_runmm_call.argtypes = [C.POINTER(RunMmConfig), vp, vp, vp, vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp,
                                            C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runmm_state_check.argtypes = [C.c_uint32, vp]
    lib.mfm_runmm_get_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.mfm_runsync_create.argtypes = [C.POINTER(vp), C.POINTER(RunSyncConfig)]
    lib.mfm_runsync_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runsync_destroy.restype = None
    lib.mfm_runsync_process_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mfm_runsync_fetch.argtypes = [vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_runsync_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runsync_get_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mfm_runsync_fetch_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runsync_store_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_hosttwin_runsync_call.argtypes = [C.POINTER(RunSyncConfig), vp, vp, vp, vp, vp, C.c_size_t, szp, vp, C.c_size_t, szp,
                                              vp, C.c_size_t, szp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runsync_state_check.argtypes = [C.c_uint32, vp]
    lib.mfm_runbatch_create.argtypes = [C.POINTER(vp), C.POINTER(RunBatchConfig)]
    lib.mfm_runbatch_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_runbatch_destroy.restype = None
    lib.mfm_runbatch_process_device.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mfm_runbatch_fetch.argtypes = [vp, vp, C.c_size_t, szp]
    lib.mfm_runbatch_device_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.mfm_runbatch_get_capacity.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.mfm_runbatch_fetch_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_runbatch_store_state.argtypes = [vp, vp, C.c_size_t]
    lib.mfm_hosttwin_runbatch_call.argtypes = [C.POINTER(RunBatchConfig), vp, vp, vp, vp, vp, vp, C.c_size_t, szp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runbatch_state_check.argtypes = [C.c_uint32, vp]
    lib.mfm_hosttwin_runflex_call.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                              C.c_size_t, szp, vp, C.c_size_t, szp, C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runpocsag_call.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_size_t, szp,
                                                C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runais_call.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_size_t, szp,
                                             C.POINTER(C.c_uint32)]
    lib.mfm_hosttwin_runrs_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_size_t, vp, vp, vp]
    lib.mfm_hosttwin_runrs_call.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, i16p, C.c_size_t, vp, i16p,
                                            vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, szp, vp, C.c_size_t, szp]
    lib.mfm_resampler_get_form.argtypes = [vp, C.POINTER(ResamplerForm)]
    lib.mfm_hosttwin_resampler_form.argtypes = [C.POINTER(ResamplerConfig), i16p, C.c_size_t, C.POINTER(ResamplerForm)]
    lib.mfm_hosttwin_resampler_matrix_block.argtypes = [C.POINTER(ResamplerConfig), i16p, C.c_size_t, C.c_uint32, i16p, C.c_size_t, i16p]
    f32p = C.POINTER(C.c_float)
    lib.mfm_f32_create.argtypes = [C.POINTER(vp), C.POINTER(F32Config)]
    lib.mfm_f32_add_channel.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.c_size_t, C.c_double]
    lib.mfm_f32_commit.argtypes = [vp]
    lib.mfm_f32_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_f32_destroy.restype = None
    lib.mfm_f32_max_out.argtypes = [vp]
    lib.mfm_f32_max_out.restype = C.c_size_t
    lib.mfm_f32_process_device.argtypes = [vp, vp, C.c_size_t, vp, C.POINTER(F32Block)]
    lib.mfm_f32_process_host.argtypes = [vp, f32p, C.c_size_t, f32p, i16p, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.mfm_mm_create.argtypes = [C.POINTER(vp), C.POINTER(MmConfig)]
    lib.mfm_mm_destroy.argtypes = [C.POINTER(vp)]
    lib.mfm_mm_destroy.restype = None
    lib.mfm_mm_max_decisions.argtypes = [vp]
    lib.mfm_mm_max_decisions.restype = C.c_size_t
    lib.mfm_mm_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(vp), C.POINTER(C.c_size_t),
                                          C.POINTER(vp)]
    lib.mfm_mm_process_host.argtypes = [vp, i16p, C.c_size_t, C.c_size_t, i16p, C.c_size_t, u32p]
    _lib = lib
    return lib


def _i16p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


class Engine:
    """One multifm channel engine (struct mfm_engine) on one GPU."""

    def __init__(self, sample_rate_hz, decimation, max_block_samples, device=0, flags=0, ext_input=None,
                 coalesce_samples=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = EngineConfig()
        cfg.abi_version = MFM_ABI_VERSION
        cfg.device = device
        cfg.sample_rate_hz = sample_rate_hz
        cfg.decimation = decimation
        cfg.max_block_samples = max_block_samples
        cfg.flags = flags
        cfg.coalesce_samples = coalesce_samples
        if ext_input is not None:
            for i, ptr in enumerate(ext_input):
                cfg.ext_input[i] = ptr
        self.sample_rate_hz, self.decimation, self.max_block_samples = sample_rate_hz, decimation, max_block_samples
        self.nr_taps = 0
        self.nr_channels = 0
        self._chk(self.lib.mfm_engine_create(C.byref(self.h), C.byref(cfg)), "mfm_engine_create")

    def _chk(self, rc, what):
        if rc < 0:
            raise MfmError(rc, what, self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
        return rc

    def close(self):
        if self.h and not getattr(self, "_borrowed", False):  # (a shard engine of a Group belongs to the group)
            self.lib.mfm_engine_destroy(C.byref(self.h))
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- channel set -------------------------------------------------------------------
    def add_channel(self, offset_hz, lpf_taps, gain=1.0, want_iq=False):
        taps = np.ascontiguousarray(lpf_taps, dtype=np.float64)
        idx = self._chk(self.lib.mfm_engine_add_channel(self.h, int(offset_hz),
                                                        taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size,
                                                        float(gain), int(want_iq)), "mfm_engine_add_channel")
        self.nr_taps = taps.size
        self.nr_channels = idx + 1
        return idx

    def add_channel_q14(self, coeff_re, coeff_im, incr, want_iq=False):
        cre = np.ascontiguousarray(coeff_re, dtype=np.int16)
        cim = np.ascontiguousarray(coeff_im, dtype=np.int16)
        idx = self._chk(self.lib.mfm_engine_add_channel_q14(self.h, _i16p(cre), _i16p(cim), cre.size,
                                                            int(incr[0]), int(incr[1]), int(want_iq)),
                        "mfm_engine_add_channel_q14")
        self.nr_taps = cre.size
        self.nr_channels = idx + 1
        return idx

    def get_channel(self, chan):
        cre = np.zeros(self.nr_taps, dtype=np.int16)
        cim = np.zeros(self.nr_taps, dtype=np.int16)
        incr = np.zeros(2, dtype=np.int16)
        self._chk(self.lib.mfm_engine_get_channel(self.h, chan, _i16p(cre), _i16p(cim), _i16p(incr)),
                  "mfm_engine_get_channel")
        return cre, cim, incr

    def commit(self):
        self._chk(self.lib.mfm_engine_commit(self.h), "mfm_engine_commit")

    # -- data path ---------------------------------------------------------------------
    def acquire_input(self):
        ptr, cap = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.mfm_engine_acquire_input(self.h, C.byref(ptr), C.byref(cap)), "mfm_engine_acquire_input")
        return ptr.value, cap.value

    def acquire_input_bytes(self, fmt):
        """where the next block goes as 8-bit IQ bytes (two per sample); MfmError(MFM_E_STATE) when the engine cannot
        read that format as bytes now"""
        ptr, cap = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.mfm_engine_acquire_input_bytes(self.h, fmt, C.byref(ptr), C.byref(cap)),
                  "mfm_engine_acquire_input_bytes")
        return ptr.value, cap.value

    def submit(self, nr_samples, producer_stream=None, wait_producer=None):
        """producer_stream: raw hipStream_t (0 = legacy default stream).  By default the engine waits for
        it whenever one is given."""
        if wait_producer is None:
            wait_producer = producer_stream is not None
        self._chk(self.lib.mfm_engine_submit(self.h, nr_samples, C.c_void_p(producer_stream or 0),
                                             int(bool(wait_producer))), "mfm_engine_submit")

    def push(self, iq):
        """iq: int16 array of interleaved I,Q (2*n elements)."""
        a = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1)
        return self.lib.mfm_engine_push(self.h, _i16p(a), a.size // 2)

    def push_bytes(self, raw, fmt):
        """raw: 8-bit IQ pairs as uint8/int8 (2*n elements) or int16 for MFM_IN_CS16; widened on the device."""
        a = np.ascontiguousarray(raw).reshape(-1)
        nr = a.size // 2
        return self.lib.mfm_engine_push_bytes(self.h, a.ctypes.data, nr, fmt)

    def fetch(self):
        """Oldest finished block as (first_output, pcm[C][n] copy, iq[C][n][2] copy or None); None when drained."""
        blk = Block()
        rc = self.lib.mfm_engine_fetch(self.h, C.byref(blk))
        if rc == MFM_E_DONE:
            return None
        self._chk(rc, "mfm_engine_fetch")
        n, stride, nch = blk.nr_outputs, blk.stride, self.nr_channels
        pcm = np.ctypeslib.as_array(blk.pcm, shape=(nch, stride))[:, :n].copy()
        iq = None
        if blk.iq:
            iq = np.ctypeslib.as_array(blk.iq, shape=(nch, stride, 2))[:, :n, :].copy()
        first = blk.first_output
        self._chk(self.lib.mfm_engine_release(self.h), "mfm_engine_release")
        return first, pcm, iq

    def run(self, iq, block_samples):
        """Push a whole stream in blocks, draining as needed.  Returns (pcm[C][N], iq[C][N][2] | None)."""
        a = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 2)
        pcm_parts, iq_parts = [], []

        def drain():
            while True:
                got = self.fetch()
                if got is None:
                    return
                pcm_parts.append(got[1])
                if got[2] is not None:
                    iq_parts.append(got[2])

        pos = 0
        while pos < a.shape[0]:
            n = min(block_samples, a.shape[0] - pos)
            rc = self.push(a[pos:pos + n])
            if rc == MFM_E_BUSY:
                drain()
                continue
            self._chk(rc, "mfm_engine_push")
            pos += n
        # a coalescing engine may hold accepted blocks it has not launched yet
        while self.flush() == MFM_E_BUSY:
            drain()
        drain()
        nch = self.nr_channels
        pcm = np.concatenate(pcm_parts, axis=1) if pcm_parts else np.zeros((nch, 0), np.int16)
        iqo = np.concatenate(iq_parts, axis=1) if iq_parts else None
        return pcm, iqo

    def last_output_device(self):
        p, st, n, q = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_void_p()
        self._chk(self.lib.mfm_engine_last_output_device(self.h, C.byref(p), C.byref(st), C.byref(n), C.byref(q)),
                  "mfm_engine_last_output_device")
        return p.value, st.value, n.value, q.value

    def flush(self):
        """launch what a coalescing engine has accepted and not launched; returns 0 or MFM_E_BUSY"""
        rc = self.lib.mfm_engine_flush(self.h)
        if rc == MFM_E_BUSY:
            return rc
        return self._chk(rc, "mfm_engine_flush")

    def replay(self, block_samples, nr_blocks):
        """nr_blocks x { acquire_input; submit(block_samples) } in C on whatever the input buffers hold"""
        self._chk(self.lib.mfm_engine_replay(self.h, block_samples, nr_blocks), "mfm_engine_replay")

    def last_launch_input(self):
        """(device address, samples, MFM_IN_* format) of what the most recent launch read"""
        p, n, f = C.c_void_p(), C.c_size_t(), C.c_int()
        self._chk(self.lib.mfm_engine_last_launch_input(self.h, C.byref(p), C.byref(n), C.byref(f)),
                  "mfm_engine_last_launch_input")
        return p.value, n.value, f.value

    def sync(self):
        self._chk(self.lib.mfm_engine_sync(self.h), "mfm_engine_sync")

    def reset(self):
        self._chk(self.lib.mfm_engine_reset(self.h), "mfm_engine_reset")

    def seek(self, outputs_before):
        """fresh history, rotators where outputs_before steps leave them, output numbering continues from there"""
        self._chk(self.lib.mfm_engine_seek(self.h, int(outputs_before)), "mfm_engine_seek")

    def stats(self):
        st = Stats()
        self._chk(self.lib.mfm_engine_get_stats(self.h, C.byref(st)), "mfm_engine_get_stats")
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def kernel_form(self):
        """before commit: the form stats() will report after it (kernel_variant, slice_channels, ...), planned on the host"""
        st = Stats()
        self._chk(self.lib.mfm_hosttwin_kernel_form(self.h, C.byref(st)), "mfm_hosttwin_kernel_form")
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def launch_ms(self, last=4096):
        """MFM_F_TIMING: durations (ms) of the most recent `last` launches, oldest first."""
        buf = np.zeros(last, np.float32)
        n = self.lib.mfm_engine_get_launch_ms(self.h, buf.ctypes.data_as(C.POINTER(C.c_float)), last)
        return buf[:n].copy()

    def launch_cycles(self, last=1024):
        """MFM_F_TIMING, second-generation kernels: (shader-clock ticks, 100 MHz reference ticks) of the most recent `last`
        launches, oldest first, as the kernel stamped them (0 where a launch left no stamp)."""
        a, b = np.zeros(last, np.uint64), np.zeros(last, np.uint64)
        n = self.lib.mfm_engine_get_launch_cycles(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   b.ctypes.data_as(C.POINTER(C.c_uint64)), last)
        return a[:n].copy(), b[:n].copy()

    @property
    def stream(self):
        return self.lib.mfm_engine_stream(self.h)


def shard_range(nr_channels, nr_shards, shard):
    """mfm_shard_range: (first, count) of a shard's contiguous channel range."""
    lib = load_library()
    lo, n = C.c_uint32(), C.c_uint32()
    lib.mfm_shard_range(nr_channels, nr_shards, shard, C.byref(lo), C.byref(n))
    return lo.value, n.value


class Group:
    """mfm_group_*: one channel set on several devices of a node (RCCL broadcast of every block)."""

    def __init__(self, sample_rate_hz, decimation, max_block_samples, devices=(0,), flags=0, exchange=MFM_X_AUTO,
                 coalesce_samples=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = GroupConfig()
        cfg.abi_version = MFM_ABI_VERSION
        cfg.nr_devices = len(devices)
        for i, d in enumerate(devices):
            cfg.devices[i] = d
        cfg.sample_rate_hz, cfg.decimation, cfg.max_block_samples = sample_rate_hz, decimation, max_block_samples
        cfg.flags, cfg.exchange = flags, exchange
        cfg.coalesce_samples = coalesce_samples
        rc = self.lib.mfm_group_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_group_create", self.lib.mfm_last_error().decode())
        self.nr_channels = 0
        self._decimation, self._sample_rate_hz, self._nr_taps = decimation, sample_rate_hz, 0

    def _chk(self, rc, what):
        if rc < 0:
            raise MfmError(rc, what, self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
        return rc

    def close(self):
        if self.h:
            self.lib.mfm_group_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_channel(self, offset_hz, lpf_taps, gain=1.0, want_iq=False):
        t = np.ascontiguousarray(lpf_taps, dtype=np.float64)
        self.nr_channels += 1
        self._nr_taps = t.size
        return self._chk(self.lib.mfm_group_add_channel(self.h, int(offset_hz), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                        t.size, float(gain), int(want_iq)), "mfm_group_add_channel")

    def commit(self):
        self._chk(self.lib.mfm_group_commit(self.h), "mfm_group_commit")
        self.nr_shards = self._chk(self.lib.mfm_group_nr_shards(self.h), "mfm_group_nr_shards")

    def shard_info(self, shard):
        lo, n, dev = C.c_uint32(), C.c_uint32(), C.c_int32()
        self._chk(self.lib.mfm_group_shard_info(self.h, shard, C.byref(lo), C.byref(n), C.byref(dev)), "mfm_group_shard_info")
        return lo.value, n.value, dev.value

    def push(self, data, fmt=MFM_IN_CS16):
        """returns 0 or MFM_E_BUSY; data: int16 [n, 2] (cs16) or uint8 [n, 2]"""
        a = np.ascontiguousarray(data)
        rc = self.lib.mfm_group_push(self.h, a.ctypes.data, a.shape[0], fmt)
        if rc == MFM_E_BUSY:
            return rc
        return self._chk(rc, "mfm_group_push")

    def fetch(self):
        """oldest finished block of all shards as one [nr_channels, n] array, or None"""
        blks = (Block * self.nr_shards)()
        rc = self.lib.mfm_group_fetch(self.h, blks)
        if rc == MFM_E_DONE:
            return None
        self._chk(rc, "mfm_group_fetch")
        parts = []
        for s in range(self.nr_shards):
            _, n, _ = self.shard_info(s)
            b = blks[s]
            arr = np.ctypeslib.as_array(b.pcm, shape=(n, b.stride))[:, :b.nr_outputs].copy()
            parts.append(arr)
        first = blks[0].first_output
        self._chk(self.lib.mfm_group_release(self.h), "mfm_group_release")
        return first, np.concatenate(parts, axis=0)

    def flush(self):
        """launch, on every shard, what has been pushed and not launched; returns 0 or MFM_E_BUSY"""
        rc = self.lib.mfm_group_flush(self.h)
        if rc == MFM_E_BUSY:
            return rc
        return self._chk(rc, "mfm_group_flush")

    def sync(self):
        self._chk(self.lib.mfm_group_sync(self.h), "mfm_group_sync")

    def stats(self, shard):
        st = Stats()
        self._chk(self.lib.mfm_group_get_stats(self.h, shard, C.byref(st)), "mfm_group_get_stats")
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def acquire_input(self):
        """(device address, capacity in samples) of where the next device-resident block goes: the root's input buffer"""
        p, cap = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.mfm_group_acquire_input(self.h, C.byref(p), C.byref(cap)), "mfm_group_acquire_input")
        return p.value, cap.value

    def submit(self, nr_samples):
        """the block at acquire_input()'s address: exchanged and submitted on every shard; returns 0 or MFM_E_BUSY"""
        rc = self.lib.mfm_group_submit(self.h, nr_samples)
        if rc == MFM_E_BUSY:
            return rc
        return self._chk(rc, "mfm_group_submit")

    def shard_engine(self, shard):
        """shard `shard`'s engine as an Engine object for the read-only calls (stats, launch_ms, launch_cycles,
        last_output_device, last_launch_input, get_channel); it does not own the handle"""
        h = self.lib.mfm_group_shard_engine(self.h, shard)
        if not h:
            raise MfmError(-1, "mfm_group_shard_engine", "no such shard")
        e = Engine.__new__(Engine)
        e.lib, e.h, e._borrowed = self.lib, C.c_void_p(h), True
        e.decimation, e.sample_rate_hz = self._decimation, self._sample_rate_hz
        e.nr_channels = self.shard_info(shard)[1]
        e.nr_taps = self._nr_taps
        return e

    def exchange_info(self):
        u, b, x = C.c_int(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.mfm_group_exchange_info(self.h, C.byref(u), C.byref(b), C.byref(x)), "mfm_group_exchange_info")
        return bool(u.value), b.value, x.value

    def exchange_detail(self, shard):
        """one shard of the exchange as measured (mfm_group_exchange_detail): dict"""
        d = ExchangeDetail()
        self._chk(self.lib.mfm_group_exchange_detail(self.h, shard, C.byref(d)), "mfm_group_exchange_detail")
        x = d.exchange_ms / d.timed_exchanges if d.timed_exchanges else None
        k = d.kernel_ms / d.timed_launches if d.timed_launches else None
        return {"device": d.device, "pci": d.pci_bus_id.decode(errors="replace"), "rccl_ranks": d.rccl_ranks,
                "exchange_ms": x, "kernel_ms": k, "timed_exchanges": d.timed_exchanges, "timed_launches": d.timed_launches,
                "bound": {0: None, 1: "kernel", 2: "exchange"}[d.bound]}


class Resampler:
    """mfm_resampler: rational resampler (+ optional DC blocker) for all channels of a PCM block."""

    def __init__(self, nr_channels, coeffs_q14, interpolate, decimate, max_in_samples, device=0, invert=False,
                 dc_pole=None, force_dot2=False):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = ResamplerConfig(MFM_ABI_VERSION, device, nr_channels, interpolate, decimate, max_in_samples,
                              int(invert), int(dc_pole is not None), float(dc_pole or 0.0),
                              MFM_RS_FORCE_DOT2 if force_dot2 else 0, 0)
        co = np.ascontiguousarray(coeffs_q14, dtype=np.int16)
        rc = self.lib.mfm_resampler_create(C.byref(self.h), C.byref(cfg), _i16p(co), co.size)
        if rc < 0:
            raise MfmError(rc, "mfm_resampler_create", self.lib.mfm_strerror(rc).decode())
        self.nr_channels = nr_channels

    def close(self):
        if self.h:
            self.lib.mfm_resampler_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_out(self):
        return self.lib.mfm_resampler_max_out(self.h)

    def form(self):
        """mfm_resampler_get_form as a dict: the kernel this resampler runs"""
        f = ResamplerForm()
        rc = self.lib.mfm_resampler_get_form(self.h, C.byref(f))
        if rc < 0:
            raise MfmError(rc, "mfm_resampler_get_form", self.lib.mfm_strerror(rc).decode())
        return f.as_dict()

    def process_host(self, pcm):
        """pcm: int16 [C][n] -> int16 [C][m]"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        cap = self.max_out()
        out = np.zeros((self.nr_channels, cap), np.int16)
        n = C.c_size_t()
        rc = self.lib.mfm_resampler_process_host(self.h, _i16p(a), a.shape[1], a.shape[1], _i16p(out), cap, C.byref(n))
        if rc < 0:
            raise MfmError(rc, "mfm_resampler_process_host", self.lib.mfm_strerror(rc).decode())
        return out[:, :n.value].copy()

    def process_device(self, d_pcm, in_stride, nr_in, stream=None):
        p, st, n = C.c_void_p(), C.c_size_t(), C.c_size_t()
        rc = self.lib.mfm_resampler_process_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0),
                                                   C.byref(p), C.byref(st), C.byref(n))
        if rc < 0:
            raise MfmError(rc, "mfm_resampler_process_device", self.lib.mfm_strerror(rc).decode())
        return p.value, st.value, n.value

    def _fail(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def process_bits_host(self, pcm, polarity):
        """pcm: int16 [C][n] -> (uint32 [C][ceil(m / 32)], m): bit j % 32 of word j / 32 is the predicate of output j
        (MFM_BITS_NEG: < 0, MFM_BITS_POS: > 0); no PCM is written.  np.unpackbits(words.view(np.uint8), bitorder="little")
        gives one byte per output."""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        cap = (self.max_out() + 31) // 32
        out = np.zeros((self.nr_channels, cap), np.uint32)
        n = C.c_size_t()
        rc = self.lib.mfm_resampler_process_bits_host(self.h, _i16p(a), a.shape[1], a.shape[1], polarity,
                                                      out.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n))
        if rc < 0:
            self._fail(rc, "mfm_resampler_process_bits_host")
        return out[:, :(n.value + 31) // 32].copy(), n.value

    def process_bits_device(self, d_pcm, in_stride, nr_in, polarity, stream=None):
        """device PCM in, BitsView out (device memory, valid until this resampler's next process call)"""
        v = BitsView()
        rc = self.lib.mfm_resampler_process_bits_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0),
                                                        polarity, C.byref(v))
        if rc < 0:
            self._fail(rc, "mfm_resampler_process_bits_device")
        return v


class F32Engine:
    """mfm_f32_*: the channel path on float32 IQ (FIR, derotation, discriminator in fp32)."""

    def __init__(self, sample_rate_hz, decimation, max_block_samples, device=0, want_iq=False, packed_fma=False,
                 tile_kernel=False):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = F32Config(MFM_ABI_VERSION, device, sample_rate_hz, decimation, max_block_samples,
                        (MFM_F32_WANT_IQ if want_iq else 0) | (MFM_F32_PACKED_FMA if packed_fma else 0) |
                        (MFM_F32_TILE_KERNEL if tile_kernel else 0))
        rc = self.lib.mfm_f32_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_f32_create", self.lib.mfm_strerror(rc).decode())
        self.want_iq = want_iq
        self.nr_channels = 0

    def _chk(self, rc, what):
        if rc < 0:
            raise MfmError(rc, what, self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
        return rc

    def close(self):
        if self.h:
            self.lib.mfm_f32_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_channel(self, offset_hz, lpf_taps, gain=1.0):
        t = np.ascontiguousarray(lpf_taps, dtype=np.float64)
        idx = self._chk(self.lib.mfm_f32_add_channel(self.h, int(offset_hz), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                     t.size, float(gain)), "mfm_f32_add_channel")
        self.nr_channels = idx + 1
        return idx

    def commit(self):
        self._chk(self.lib.mfm_f32_commit(self.h), "mfm_f32_commit")

    def max_out(self):
        return self.lib.mfm_f32_max_out(self.h)

    def process_host(self, iq):
        """iq: float32 [n][2] (or flat interleaved) -> (pcm_f32 [C][m], pcm_i16 [C][m], iq_f32 [C][m][2] or None)"""
        a = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        n_in = a.size // 2
        cap = self.max_out()
        Cn = self.nr_channels
        pf = np.zeros((Cn, cap), np.float32)
        pi = np.zeros((Cn, cap), np.int16)
        qf = np.zeros((Cn, cap, 2), np.float32) if self.want_iq else None
        n = C.c_size_t()
        f32p = C.POINTER(C.c_float)
        self._chk(self.lib.mfm_f32_process_host(self.h, a.ctypes.data_as(f32p), n_in, pf.ctypes.data_as(f32p), _i16p(pi),
                                                qf.ctypes.data_as(f32p) if qf is not None else None, cap, C.byref(n)),
                  "mfm_f32_process_host")
        m = n.value
        return pf[:, :m].copy(), pi[:, :m].copy(), (qf[:, :m].copy() if qf is not None else None)

    def process_device(self, d_iq, nr_samples, stream=None):
        b = F32Block()
        self._chk(self.lib.mfm_f32_process_device(self.h, C.c_void_p(d_iq), nr_samples, C.c_void_p(stream or 0),
                                                  C.byref(b)), "mfm_f32_process_device")
        return b


class MuellerMuller:
    """mfm_mm_*: Mueller-Muller clock recovery (pager/mueller_muller.c) for all channels of a PCM block."""

    def __init__(self, nr_channels, kw, km, samples_per_bit, error_min, error_max, max_in_samples, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = MmConfig(MFM_ABI_VERSION, device, nr_channels, max_in_samples, kw, km, samples_per_bit, error_min,
                       error_max)
        rc = self.lib.mfm_mm_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_mm_create", self.lib.mfm_strerror(rc).decode())
        self.nr_channels = nr_channels

    def close(self):
        if self.h:
            self.lib.mfm_mm_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_host(self, pcm, nr_in):
        """pcm: int16 [C][stride] with stride > nr_in when the look-ahead sample is there -> list of per-channel
        decision arrays"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        cap = self.lib.mfm_mm_max_decisions(self.h)
        dec = np.zeros((self.nr_channels, cap), np.int16)
        cnt = np.zeros(self.nr_channels, np.uint32)
        rc = self.lib.mfm_mm_process_host(self.h, _i16p(a), a.shape[1], nr_in, _i16p(dec), cap,
                                          cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc < 0:
            raise MfmError(rc, "mfm_mm_process_host", self.lib.mfm_strerror(rc).decode())
        return [dec[c, :cnt[c]].copy() for c in range(self.nr_channels)]

    def process_device(self, d_pcm, in_stride, nr_in, stream=None):
        """resident PCM -> (device pointer of the decisions, their row stride, device pointer of the counts)"""
        d_dec, stride, d_cnt = C.c_void_p(), C.c_size_t(), C.c_void_p()
        rc = self.lib.mfm_mm_process_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0),
                                            C.byref(d_dec), C.byref(stride), C.byref(d_cnt))
        if rc < 0:
            raise MfmError(rc, "mfm_mm_process_device", self.lib.mfm_strerror(rc).decode())
        return d_dec.value, stride.value, d_cnt.value


class Pocsag:
    """mfm_pocsag: POCSAG slicer / sync / batch collection + BCH(31,21) for all channels of a 38 400 Hz PCM block."""

    def __init__(self, nr_channels, max_in_samples, device=0, max_events=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = PocsagConfig(MFM_ABI_VERSION, device, nr_channels, max_in_samples, max_events, 0)
        rc = self.lib.mfm_pocsag_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_create", self.lib.mfm_strerror(rc).decode())
        self.nr_channels = nr_channels
        self.max_events = max_events or (max_in_samples // 2048 + 16)

    def close(self):
        if self.h:
            self.lib.mfm_pocsag_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_host(self, pcm):
        """pcm: int16 [C][n]; returns the events of this call as a structured array (POCSAG_EVENT_DTYPE)"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        rc = self.lib.mfm_pocsag_process_host(self.h, _i16p(a), a.shape[1], a.shape[1])
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_process_host", self.lib.mfm_strerror(rc).decode())
        return self.fetch_events()

    def process_device(self, d_pcm, in_stride, nr_in, stream=None):
        rc = self.lib.mfm_pocsag_process_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_process_device", self.lib.mfm_strerror(rc).decode())

    def process_bits_device(self, view, stream=None):
        """as process_device with nr_in = view.nr_bits, from a Resampler's MFM_BITS_NEG BitsView instead of PCM"""
        rc = self.lib.mfm_pocsag_process_bits_device(self.h, C.byref(view), C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_process_bits_device", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def seek(self, samples_before):
        """mfm_pocsag_seek: a fresh stage whose next sample has index samples_before (added to every event's sample)"""
        rc = self.lib.mfm_pocsag_seek(self.h, int(samples_before))
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_seek", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def fetch_events(self):
        cap = self.nr_channels * self.max_events
        out = np.zeros(cap, POCSAG_EVENT_DTYPE)
        n = C.c_size_t()
        rc = self.lib.mfm_pocsag_fetch_events(self.h, out.ctypes.data, cap, C.byref(n))
        if rc < 0:
            raise MfmError(rc, "mfm_pocsag_fetch_events", self.lib.mfm_strerror(rc).decode())
        return out[:n.value].copy()


class Ais:
    """mfm_ais: AIS slicer / preamble detector / NRZI + HDLC bit recovery / FCS check for all channels of a 48 000 Hz
    PCM block.  One event per candidate packet (AIS_EVENT_DTYPE), CRC rejects included (fcs_valid = 0)."""

    def __init__(self, nr_channels, max_in_samples, device=0, max_events=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = AisConfig(MFM_ABI_VERSION, device, nr_channels, max_in_samples, max_events, 0)
        rc = self.lib.mfm_ais_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_ais_create", self.lib.mfm_strerror(rc).decode())
        self.nr_channels = nr_channels
        self.max_events = max_events or (max_in_samples // 160 + 16)

    def close(self):
        if self.h:
            self.lib.mfm_ais_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_host(self, pcm):
        """pcm: int16 [C][n]; returns the events of this call as a structured array (AIS_EVENT_DTYPE)"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        rc = self.lib.mfm_ais_process_host(self.h, _i16p(a), a.shape[1], a.shape[1])
        if rc < 0:
            raise MfmError(rc, "mfm_ais_process_host", self.lib.mfm_strerror(rc).decode())
        return self.fetch_events()

    def process_device(self, d_pcm, in_stride, nr_in, stream=None):
        rc = self.lib.mfm_ais_process_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_ais_process_device", self.lib.mfm_strerror(rc).decode())

    def process_bits_device(self, view, stream=None):
        """as process_device with nr_in = view.nr_bits, from a Resampler's MFM_BITS_POS BitsView instead of PCM"""
        rc = self.lib.mfm_ais_process_bits_device(self.h, C.byref(view), C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_ais_process_bits_device", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def seek(self, samples_before):
        """mfm_ais_seek: a fresh stage whose next sample has index samples_before (added to sample and start_sample)"""
        rc = self.lib.mfm_ais_seek(self.h, int(samples_before))
        if rc < 0:
            raise MfmError(rc, "mfm_ais_seek", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def fetch_events(self):
        cap = self.nr_channels * self.max_events
        out = np.zeros(cap, AIS_EVENT_DTYPE)
        n = C.c_size_t()
        rc = self.lib.mfm_ais_fetch_events(self.h, out.ctypes.data, cap, C.byref(n))
        if rc < 0:
            raise MfmError(rc, "mfm_ais_fetch_events", self.lib.mfm_strerror(rc).decode())
        return out[:n.value].copy()


class Level:
    """mfm_level: per-channel signal level (energy, wrapped-difference energy, peak) over windows of `window_samples`
    samples and a squelch stepped once per window, for all channels of a block of PCM (form MFM_LEVEL_PCM) or filtered-IQ
    (MFM_LEVEL_IQ) rows.  One record per channel and completed window (LEVEL_RECORD_DTYPE)."""

    def __init__(self, nr_channels, max_in_samples, window_samples, form=MFM_LEVEL_PCM, metric=MFM_LEVEL_METRIC_ENERGY,
                 sense=MFM_LEVEL_OPEN_ABOVE, open_thr=0, close_thr=0, hang_windows=0, device=0, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = LevelConfig(abi_version, device, nr_channels, max_in_samples, form, window_samples, metric, sense,
                          int(open_thr), int(close_thr), hang_windows, 0)
        rc = self.lib.mfm_level_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_level_create", (self.lib.mfm_last_error() if rc == MFM_E_INVAL else self.lib.mfm_strerror(rc)).decode())
        self.nr_channels = nr_channels
        self.elems = 2 if form == MFM_LEVEL_IQ else 1

    def close(self):
        if self.h:
            self.lib.mfm_level_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_host(self, rows):
        """rows: int16 [C][n] (PCM form) or [C][n][2] / [C][2 n] (IQ form); returns the records of this call, [C][windows]"""
        a = np.ascontiguousarray(rows, dtype=np.int16).reshape(self.nr_channels, -1)
        rc = self.lib.mfm_level_process_host(self.h, _i16p(a), a.shape[1], a.shape[1] // self.elems)
        if rc < 0:
            raise MfmError(rc, "mfm_level_process_host", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
        return self.fetch()

    def process_device(self, d_rows, in_stride, nr_in, stream=None):
        """in_stride counts int16 elements in both forms (the engine's IQ rows: 2 * stride)"""
        rc = self.lib.mfm_level_process_device(self.h, C.c_void_p(d_rows), in_stride, nr_in, C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_level_process_device", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def seek(self, samples_before):
        """mfm_level_seek: a fresh stage whose next sample has index samples_before, a multiple of window_samples"""
        rc = self.lib.mfm_level_seek(self.h, int(samples_before))
        if rc < 0:
            raise MfmError(rc, "mfm_level_seek", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def fetch(self, max_records=None):
        """the last call's records as a structured array [C][windows]; with max_records too small: MfmError(MFM_E_NOMEM)
        whose `needed` attribute is the record count that would fit"""
        n = C.c_size_t()
        if max_records is None:
            rc = self.lib.mfm_level_fetch(self.h, None, 0, C.byref(n))
            if rc not in (MFM_OK, MFM_E_NOMEM):
                raise MfmError(rc, "mfm_level_fetch", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
            max_records = self.nr_channels * n.value
        out = np.zeros(max(max_records, 1), LEVEL_RECORD_DTYPE)
        rc = self.lib.mfm_level_fetch(self.h, out.ctypes.data, max_records, C.byref(n))
        if rc < 0:
            err = MfmError(rc, "mfm_level_fetch", self.lib.mfm_strerror(rc).decode())
            err.needed = self.nr_channels * n.value
            err.buffer = out
            raise err
        return out[:self.nr_channels * n.value].reshape(self.nr_channels, n.value).copy()

    def device_view(self):
        """(d_records, record_stride, nr_windows, d_open): device addresses of the last call's records and of the per-channel
        squelch state (uint32 each)"""
        rec, st, n, op = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_void_p()
        rc = self.lib.mfm_level_device_view(self.h, C.byref(rec), C.byref(st), C.byref(n), C.byref(op))
        if rc < 0:
            raise MfmError(rc, "mfm_level_device_view", self.lib.mfm_strerror(rc).decode())
        return rec.value, st.value, n.value, op.value

    def set_adaptive(self, floor_windows=None, open_q8=0, close_q8=0, warmup_windows=0, flags=0, reserved=0):
        """mfm_level_set_adaptive: the squelch on ratios (in 1/256) to the channel's own noise floor over the last floor_windows
        windows; floor_windows None switches it off.  Only on a fresh object (after create or seek, before the next call)"""
        a = None if floor_windows is None else LevelAdaptive(floor_windows, open_q8, close_q8, warmup_windows, flags, reserved)
        rc = self.lib.mfm_level_set_adaptive(self.h, C.byref(a) if a is not None else None)
        if rc < 0:
            raise MfmError(rc, "mfm_level_set_adaptive", (self.lib.mfm_last_error() if rc == MFM_E_INVAL else self.lib.mfm_strerror(rc)).decode())

    def get_adaptive(self):
        """mfm_level_get_adaptive: None when off, else dict(floor_windows, open_q8, close_q8, warmup_windows)"""
        on, a = C.c_uint32(), LevelAdaptive()
        rc = self.lib.mfm_level_get_adaptive(self.h, C.byref(on), C.byref(a))
        if rc < 0:
            raise MfmError(rc, "mfm_level_get_adaptive", self.lib.mfm_strerror(rc).decode())
        if not on.value:
            return None
        return dict(floor_windows=a.floor_windows, open_q8=a.open_q8, close_q8=a.close_q8, warmup_windows=a.warmup_windows)

    def fetch_floor(self, max_values=None):
        """the floors of the last call's windows, uint64 [C][windows]; with max_values too small: MfmError(MFM_E_NOMEM) whose
        `needed` attribute is the count that would fit"""
        n = C.c_size_t()
        if max_values is None:
            rc = self.lib.mfm_level_fetch_floor(self.h, None, 0, C.byref(n))
            if rc not in (MFM_OK, MFM_E_NOMEM):
                raise MfmError(rc, "mfm_level_fetch_floor", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())
            max_values = self.nr_channels * n.value
        out = np.zeros(max(max_values, 1), np.uint64)
        rc = self.lib.mfm_level_fetch_floor(self.h, out.ctypes.data, max_values, C.byref(n))
        if rc < 0:
            err = MfmError(rc, "mfm_level_fetch_floor", (self.lib.mfm_last_error() if rc == MFM_E_INVAL else self.lib.mfm_strerror(rc)).decode())
            err.needed = self.nr_channels * n.value
            err.buffer = out
            raise err
        return out[:self.nr_channels * n.value].reshape(self.nr_channels, n.value).copy()

    def floor_view(self):
        """(d_floor, floor_stride): the device address of the last call's floors, d_floor[channel * floor_stride + i]"""
        fl, st = C.c_void_p(), C.c_size_t()
        rc = self.lib.mfm_level_floor_view(self.h, C.byref(fl), C.byref(st))
        if rc < 0:
            raise MfmError(rc, "mfm_level_floor_view", (self.lib.mfm_last_error() if rc == MFM_E_INVAL else self.lib.mfm_strerror(rc)).decode())
        return fl.value, st.value


def hosttwin_level_adaptive(metric, sense, open_thr, close_thr, hang_windows, floor_windows, open_q8, close_q8, warmup_windows=0):
    """mfm_hosttwin_level_adaptive for one channel: metric uint64 [n], the windows from the first after create or seek on;
    returns (floor uint64 [n], open uint32 [n])"""
    lib = load_library()
    m = np.ascontiguousarray(metric, dtype=np.uint64).reshape(-1)
    n = m.size
    buf = m if n else np.zeros(1, np.uint64)
    fl, op = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
    a = LevelAdaptive(floor_windows, open_q8, close_q8, warmup_windows, 0, 0)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.mfm_hosttwin_level_adaptive(buf.ctypes.data_as(u64p), n, sense, int(open_thr), int(close_thr), hang_windows, C.byref(a),
                                    fl.ctypes.data_as(u64p), op.ctypes.data_as(u32p))
    return fl[:n], op[:n]


def hosttwin_level_window(x, form=MFM_LEVEL_PCM, prev=0):
    """mfm_hosttwin_level_window: (energy, diff_energy, peak) of one window; x int16 [n] (PCM) or [n][2] (IQ)"""
    lib = load_library()
    a = np.ascontiguousarray(x, dtype=np.int16).reshape(-1)
    n = a.size // (2 if form == MFM_LEVEL_IQ else 1)
    e, d, p = C.c_uint64(), C.c_uint64(), C.c_uint32()
    buf = a if a.size else np.zeros(1, np.int16)
    lib.mfm_hosttwin_level_window(_i16p(buf), n, form, int(prev), C.byref(e), C.byref(d), C.byref(p))
    return e.value, d.value, p.value


def hosttwin_squelch_step(sense, open_thr, close_thr, hang_windows, metric, open_, bad):
    """mfm_hosttwin_squelch_step: one window's step; returns the new (open, bad)"""
    lib = load_library()
    o, b = C.c_uint32(int(open_)), C.c_uint32(int(bad))
    lib.mfm_hosttwin_squelch_step(sense, int(open_thr), int(close_thr), hang_windows, int(metric), C.byref(o), C.byref(b))
    return o.value, b.value


class Gate:
    """mfm_gate: of a block of PCM (elems_per_sample 1) or filtered-IQ (2) rows, the windows that a Level's records call open,
    packed into one dense payload with a run list (GATE_RUN_DTYPE).  Fed the same nr_in sequence as that Level."""

    def __init__(self, nr_channels, max_in_samples, window_samples, elems_per_sample=1, max_open_windows=0, device=0,
                 abi_version=MFM_ABI_VERSION, preroll_windows=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = GateConfig(abi_version, device, nr_channels, max_in_samples, window_samples, elems_per_sample, max_open_windows, 0)
        rc = self.lib.mfm_gate_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_gate_create", (self.lib.mfm_last_error() if rc == MFM_E_INVAL else self.lib.mfm_strerror(rc)).decode())
        self.nr_channels = nr_channels
        self.elems = elems_per_sample
        if preroll_windows:
            try:
                self.set_preroll(preroll_windows)
            except MfmError:
                self.close()
                raise

    def set_preroll(self, preroll_windows):
        """mfm_gate_set_preroll: window k goes out when any record k .. k + P is open, P windows late; before the first call only"""
        rc = self.lib.mfm_gate_set_preroll(self.h, preroll_windows)
        if rc < 0:
            self._raise(rc, "mfm_gate_set_preroll")

    def flush_device(self, stream=None):
        """mfm_gate_flush_device: end of the stream; the windows pre-roll still held back are the result fetch() returns"""
        rc = self.lib.mfm_gate_flush_device(self.h, C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_gate_flush_device")

    def seek(self, samples_before):
        """mfm_gate_seek: a fresh gate with the same pre-roll whose next sample has index samples_before, a multiple of window_samples"""
        rc = self.lib.mfm_gate_seek(self.h, int(samples_before))
        if rc < 0:
            raise MfmError(rc, "mfm_gate_seek", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def close(self):
        if self.h:
            self.lib.mfm_gate_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE, MFM_E_DEVICE)
                       else self.lib.mfm_strerror(rc).decode())

    def process_host(self, rows, records):
        """rows: int16 [C][n] or [C][n][2] / [C][2 n] (two elements per sample); records: LEVEL_RECORD_DTYPE [C][windows] of the
        same block; returns (runs, payload) of this call"""
        a = np.ascontiguousarray(rows, dtype=np.int16).reshape(self.nr_channels, -1)
        r = np.ascontiguousarray(records, dtype=LEVEL_RECORD_DTYPE).reshape(self.nr_channels, -1)
        rc = self.lib.mfm_gate_process_host(self.h, _i16p(a), a.shape[1], a.shape[1] // self.elems, r.ctypes.data, r.shape[1], r.shape[1])
        if rc < 0:
            self._raise(rc, "mfm_gate_process_host")
        return self.fetch()

    def process_device(self, d_rows, in_stride, nr_in, d_records, record_stride, nr_windows, stream=None):
        """d_records, record_stride, nr_windows: the first three of Level.device_view() for the same block; in_stride counts
        int16 elements (the engine's IQ rows: 2 * stride)"""
        rc = self.lib.mfm_gate_process_device(self.h, C.c_void_p(d_rows), in_stride, nr_in, C.c_void_p(d_records), record_stride,
                                              nr_windows, C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_gate_process_device")

    def fetch(self, max_runs=None, max_elems=None):
        """(runs, payload) of the last call: GATE_RUN_DTYPE [nr_runs] and int16 [nr_elems].  With max_runs or max_elems too small:
        MfmError(MFM_E_NOMEM) whose `needed` attribute is the (runs, elements) that would fit"""
        nr, ne = C.c_size_t(), C.c_size_t()
        if max_runs is None or max_elems is None:
            rc = self.lib.mfm_gate_fetch(self.h, None, 0, C.byref(nr), None, 0, C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffers
                self._raise(rc, "mfm_gate_fetch")
            max_runs = nr.value if max_runs is None else max_runs
            max_elems = ne.value if max_elems is None else max_elems
        runs = np.zeros(max(max_runs, 1), GATE_RUN_DTYPE)
        payload = np.zeros(max(max_elems, 1), np.int16)
        rc = self.lib.mfm_gate_fetch(self.h, runs.ctypes.data, max_runs, C.byref(nr), payload.ctypes.data, max_elems, C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_gate_fetch")
            except MfmError as err:
                err.needed = (nr.value, ne.value)
                err.buffers = (runs, payload)
                raise
        return runs[:nr.value].copy(), payload[:ne.value].copy()

    def device_view(self):
        """(d_runs, d_payload, d_totals): device addresses of the last call's runs, payload and the four uint64 totals
        (runs, payload elements, overflow, out of step)"""
        r, p, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_gate_device_view(self.h, C.byref(r), C.byref(p), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_gate_device_view")
        return r.value, p.value, t.value


def hosttwin_gate_call(window_samples, elems_per_sample, pos, rows, carry, records, max_runs=None, max_elems=None):
    """mfm_hosttwin_gate_call: one call of the gate on the CPU.  rows int16 [C][n * elems_per_sample], carry int16
    [C][window_samples * elems_per_sample] (updated in place), records LEVEL_RECORD_DTYPE [C][windows]; returns (runs, payload)"""
    lib = load_library()
    carry = np.asarray(carry)
    assert carry.dtype == np.int16 and carry.flags.c_contiguous
    nch = carry.shape[0]
    a = np.ascontiguousarray(rows, dtype=np.int16).reshape(nch, -1)
    r = np.ascontiguousarray(records, dtype=LEVEL_RECORD_DTYPE).reshape(nch, -1)
    nw = r.shape[1]
    max_runs = nch * ((nw + 1) // 2) if max_runs is None else max_runs
    max_elems = nch * nw * window_samples * elems_per_sample if max_elems is None else max_elems
    runs = np.zeros(max(max_runs, 1), GATE_RUN_DTYPE)
    payload = np.zeros(max(max_elems, 1), np.int16)
    nr, ne = C.c_size_t(), C.c_size_t()
    abuf = a if a.size else np.zeros((nch, 1), np.int16)
    rc = lib.mfm_hosttwin_gate_call(nch, window_samples, elems_per_sample, int(pos), _i16p(abuf), a.shape[1], a.shape[1] // elems_per_sample,
                                    _i16p(carry), r.ctypes.data, nw, nw, runs.ctypes.data, max_runs, C.byref(nr), payload.ctypes.data,
                                    max_elems, C.byref(ne))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_gate_call", lib.mfm_last_error().decode() if rc == MFM_E_STATE else lib.mfm_strerror(rc).decode())
        err.needed = (nr.value, ne.value)
        raise err
    return runs[:nr.value].copy(), payload[:ne.value].copy()


def hosttwin_gate_call_preroll(window_samples, elems_per_sample, preroll_windows, pos, rows, history, open_bits, records, flush=False,
                               max_runs=None, max_elems=None):
    """mfm_hosttwin_gate_call_preroll: one call, or with flush the flush (rows and records empty), of a gate with pre-roll on the
    CPU.  history int16 [C][(P + 1) * window_samples * elems_per_sample] and open_bits uint64 [C] are the stage's state, zero
    at pos 0 and updated in place; returns (runs, payload)"""
    lib = load_library()
    history, open_bits = np.asarray(history), np.asarray(open_bits)
    assert history.dtype == np.int16 and history.flags.c_contiguous and open_bits.dtype == np.uint64 and open_bits.flags.c_contiguous
    nch = history.shape[0]
    we = window_samples * elems_per_sample
    assert history.shape[1] == (preroll_windows + 1) * we and open_bits.shape == (nch,)
    a = np.ascontiguousarray(rows, dtype=np.int16).reshape(nch, -1)
    r = np.ascontiguousarray(records, dtype=LEVEL_RECORD_DTYPE).reshape(nch, -1)
    nw = r.shape[1]
    most = preroll_windows if flush else nw
    max_runs = nch * ((most + 1) // 2) if max_runs is None else max_runs
    max_elems = nch * most * we if max_elems is None else max_elems
    runs = np.zeros(max(max_runs, 1), GATE_RUN_DTYPE)
    payload = np.zeros(max(max_elems, 1), np.int16)
    nr, ne = C.c_size_t(), C.c_size_t()
    abuf = a if a.size else np.zeros((nch, 1), np.int16)
    rc = lib.mfm_hosttwin_gate_call_preroll(nch, window_samples, elems_per_sample, preroll_windows, int(pos), int(bool(flush)), _i16p(abuf),
                                            a.shape[1], a.shape[1] // elems_per_sample, _i16p(history), open_bits.ctypes.data,
                                            r.ctypes.data, nw, nw, runs.ctypes.data, max_runs, C.byref(nr), payload.ctypes.data, max_elems,
                                            C.byref(ne))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_gate_call_preroll",
                       lib.mfm_last_error().decode() if rc == MFM_E_STATE else lib.mfm_strerror(rc).decode())
        err.needed = (nr.value, ne.value)
        raise err
    return runs[:nr.value].copy(), payload[:ne.value].copy()


def runrs_phase_len(nr_coeffs, interpolate):
    """taps per phase (csrc/mfm_rs_plan.h): ceil(nr_coeffs / interpolate) rounded up to a multiple of 4"""
    return ((nr_coeffs + interpolate - 1) // interpolate + 3) & ~3


class RunResampler:
    """mfm_runrs: the runs of a Gate's device view through the rational resampler, one fresh resampler per stretch of
    consecutive windows of a channel; one RUNRS_RUN_DTYPE per gate run and a dense int16 payload.  max_windows / max_runs 0
    take the defaults of a Gate made from the same nr_channels, max_in_samples, window_samples and preroll_windows."""

    def __init__(self, nr_channels, coeffs_q14, interpolate, decimate, window_samples, max_in_samples=0, preroll_windows=0,
                 max_windows=0, max_runs=0, invert=False, device=0, flags=0, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = RunrsConfig(abi_version, device, nr_channels, interpolate, decimate, window_samples, max_windows, max_runs, int(invert),
                          flags, max_in_samples, preroll_windows)
        co = np.ascontiguousarray(coeffs_q14, dtype=np.int16)
        rc = self.lib.mfm_runrs_create(C.byref(self.h), C.byref(cfg), _i16p(co) if co.size else None, co.size)
        if rc < 0:
            self._raise(rc, "mfm_runrs_create")
        self.nr_channels = nr_channels
        self.plen = runrs_phase_len(co.size, interpolate)

    def close(self):
        if self.h:
            self.lib.mfm_runrs_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of Gate.device_view(), after the gate's process_device or flush_device on the same stream"""
        rc = self.lib.mfm_runrs_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runrs_process_device")

    def fetch(self, max_runs=None, max_elems=None):
        """(runs, payload) of the last call: RUNRS_RUN_DTYPE [nr_runs] and int16 [nr_elems].  With max_runs or max_elems too
        small: MfmError(MFM_E_NOMEM) whose `needed` attribute is the (runs, elements) that would fit"""
        nr, ne = C.c_size_t(), C.c_size_t()
        if max_runs is None or max_elems is None:
            rc = self.lib.mfm_runrs_fetch(self.h, None, 0, C.byref(nr), None, 0, C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffers
                self._raise(rc, "mfm_runrs_fetch")
            max_runs = nr.value if max_runs is None else max_runs
            max_elems = ne.value if max_elems is None else max_elems
        runs = np.zeros(max(max_runs, 1), RUNRS_RUN_DTYPE)
        payload = np.zeros(max(max_elems, 1), np.int16)
        rc = self.lib.mfm_runrs_fetch(self.h, runs.ctypes.data, max_runs, C.byref(nr), payload.ctypes.data, max_elems, C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runrs_fetch")
            except MfmError as err:
                err.needed = (nr.value, ne.value)
                err.buffers = (runs, payload)
                raise
        return runs[:nr.value].copy(), payload[:ne.value].copy()

    def device_view(self):
        """(d_runs, d_payload, d_totals): device addresses of the last call's runs, payload and the four uint64 totals
        (runs, output elements, overflow, gate error)"""
        r, p, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runrs_device_view(self.h, C.byref(r), C.byref(p), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runrs_device_view")
        return r.value, p.value, t.value

    def process_bits_device(self, d_runs, d_payload, d_totals, polarity, stream=None):
        """as process_device, with one predicate bit per output (MFM_BITS_NEG: sample < 0, MFM_BITS_POS: sample > 0) in the
        place of the int16; the result is read with bits_view() or fetch_bits()"""
        rc = self.lib.mfm_runrs_process_bits_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), polarity,
                                                    C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runrs_process_bits_device")

    def process_view_device(self, d_runs, d_payload, d_totals, d_payload_elems, stream=None):
        """mfm_runrs_process_view_device: as process_device behind a local route of the run router, RunRouter(local=True): the
        three addresses of its device_view(route) and the address of its bound_view().  A run's payload range is checked against
        the uint64 at d_payload_elems (how much payload exists); the totals' elements are only the load that must fit the capacity"""
        rc = self.lib.mfm_runrs_process_view_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals),
                                                    C.c_void_p(d_payload_elems), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runrs_process_view_device")

    def process_bits_view_device(self, d_runs, d_payload, d_totals, d_payload_elems, polarity, stream=None):
        """mfm_runrs_process_bits_view_device: process_bits_device with the bound of process_view_device"""
        rc = self.lib.mfm_runrs_process_bits_view_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals),
                                                         C.c_void_p(d_payload_elems), polarity, C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runrs_process_bits_view_device")

    def bits_view(self):
        """RunrsBitsView of the last (bits) call: device addresses of its runs (out_offset in words), bit payload and totals"""
        v = RunrsBitsView()
        rc = self.lib.mfm_runrs_bits_view(self.h, C.byref(v))
        if rc < 0:
            self._raise(rc, "mfm_runrs_bits_view")
        return v

    def fetch_bits(self, max_runs=None, max_words=None):
        """(runs, bits) of the last (bits) call: RUNRS_RUN_DTYPE [nr_runs] with out_offset in words, and uint32 [nr_words].
        Errors as fetch()"""
        nr, nw = C.c_size_t(), C.c_size_t()
        if max_runs is None or max_words is None:
            rc = self.lib.mfm_runrs_fetch_bits(self.h, None, 0, C.byref(nr), None, 0, C.byref(nw))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffers
                self._raise(rc, "mfm_runrs_fetch_bits")
            max_runs = nr.value if max_runs is None else max_runs
            max_words = nw.value if max_words is None else max_words
        runs = np.zeros(max(max_runs, 1), RUNRS_RUN_DTYPE)
        bits = np.zeros(max(max_words, 1), np.uint32)
        rc = self.lib.mfm_runrs_fetch_bits(self.h, runs.ctypes.data, max_runs, C.byref(nr), bits.ctypes.data, max_words, C.byref(nw))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runrs_fetch_bits")
            except MfmError as err:
                err.needed = (nr.value, nw.value)
                err.buffers = (runs, bits)
                raise
        return runs[:nr.value].copy(), bits[:nw.value].copy()

    def bits_capacity(self):
        """(max_runs, max_words) of the bits form: max_words = max_out_elems // 32 + max_runs"""
        nr, nw = C.c_uint32(), C.c_uint64()
        rc = self.lib.mfm_runrs_get_bits_capacity(self.h, C.byref(nr), C.byref(nw))
        if rc < 0:
            self._raise(rc, "mfm_runrs_get_bits_capacity")
        return nr.value, nw.value

    def capacity(self):
        """(max_runs, max_out_elems): the most runs and output elements one call can produce, which a stage behind sizes
        itself from"""
        nr, ne = C.c_uint32(), C.c_uint64()
        rc = self.lib.mfm_runrs_get_capacity(self.h, C.byref(nr), C.byref(ne))
        if rc < 0:
            self._raise(rc, "mfm_runrs_get_capacity")
        return nr.value, ne.value

    def set_dc_block(self, pole):
        """mfm_runrs_set_dc_block: the DC blocker (decoder -b) with this pole behind the resampler, one fresh blocker per
        stretch; None switches it off.  Only before the first process call"""
        rc = self.lib.mfm_runrs_set_dc_block(self.h, int(pole is not None), float(pole if pole is not None else 0.0))
        if rc < 0:
            self._raise(rc, "mfm_runrs_set_dc_block")

    def dc_block(self):
        """(on, dc_p): whether the DC blocker is on, and its (1 - pole) in Q14 (0 when off)"""
        on, p = C.c_uint32(), C.c_int32()
        rc = self.lib.mfm_runrs_get_dc_block(self.h, C.byref(on), C.byref(p))
        if rc < 0:
            self._raise(rc, "mfm_runrs_get_dc_block")
        return bool(on.value), p.value

    def fetch_state(self):
        """mfm_runrs_fetch_state: (state, pending) as hosttwin_runrs_state has them, RUNRS_STATE_DTYPE [C] and int16 [C][plen], and
        with the DC blocker on (state, pending, dc), dc RUNRS_DC_STATE_DTYPE [C]: what the host twins carry"""
        dc_on = self.dc_block()[0]
        state = np.zeros(self.nr_channels, RUNRS_STATE_DTYPE)
        pending = np.zeros((self.nr_channels, self.plen), np.int16)
        dc = np.zeros(self.nr_channels, RUNRS_DC_STATE_DTYPE) if dc_on else None
        rc = self.lib.mfm_runrs_fetch_state(self.h, state.ctypes.data, pending.ctypes.data, dc.ctypes.data if dc_on else None,
                                            self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runrs_fetch_state")
        return (state, pending, dc) if dc_on else (state, pending)

    def store_state(self, state, pending, dc=None, nr_channels=None):
        """mfm_runrs_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written.  dc is required with the DC blocker on, None with it off"""
        st = np.ascontiguousarray(state, dtype=RUNRS_STATE_DTYPE) if state is not None else None
        pe = np.ascontiguousarray(pending, dtype=np.int16) if pending is not None else None
        d = np.ascontiguousarray(dc, dtype=RUNRS_DC_STATE_DTYPE) if dc is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        assert pe is None or pe.shape == (n, self.plen)
        assert d is None or d.shape == (n,)
        rc = self.lib.mfm_runrs_store_state(self.h, st.ctypes.data if st is not None else None, pe.ctypes.data if pe is not None else None,
                                            d.ctypes.data if d is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runrs_store_state")


def _route_table(route_of_channel):
    t = np.ascontiguousarray(route_of_channel, dtype=np.uint8).reshape(-1)
    return t, (t.ctypes.data if t.size else None)


class RunRouter:
    """mfm_runroute: the runs of a Gate's device view partitioned by a per-channel route table (a route below nr_routes, or
    MFM_ROUTE_NONE), so that one gate feeds a burst chain per protocol.  Zero-copy: device_view(route) is that route's run list
    with the gate's payload pointer, and goes where Gate.device_view() goes.  A route's RunResampler is made with the whole
    gate's numbers (all channels): channel numbers stay global.

    With sets= in the place of route_of_channel (mfm_runroute_create_sets) a channel's byte is a set of routes, bit k = route k, so a
    channel may feed several chains.  pack=True (MFM_RUNROUTE_F_PACK, sets form only) gives every route route-local channel
    numbers and a dense payload of its own: route_caps(k) are the numbers its RunResampler is made with, route_channels(k) maps
    its local channels back, fetch_payload(k) reads its payload.

    local=True (mfm_runroute_create_local, with sets=, never with pack) gives pack's route-local channel numbers and route_caps()
    on the gate's payload in place: nothing is copied, device_view(k) carries the gate's payload pointer and the route's own
    load, and a route's RunResampler takes it through process_view_device / process_bits_view_device with bound_view()."""

    def __init__(self, route_of_channel=None, nr_routes=0, window_samples=0, max_in_samples=0, preroll_windows=0, max_windows=0, max_runs=0,
                 device=0, flags=0, abi_version=MFM_ABI_VERSION, nr_channels=None, sets=None, pack=False, local=False):
        self.lib = load_library()
        self.h = C.c_void_p()
        if sets is not None and route_of_channel is not None:
            raise ValueError("RunRouter takes route_of_channel or sets=, not both")
        if pack and sets is None:
            raise ValueError("pack=True needs sets=: mfm_runroute_create takes no flags")
        if local and (sets is None or pack):
            raise ValueError("local=True needs sets= and excludes pack=True: mfm_runroute_create_local takes a table of sets and no flags")
        table, ptr = _route_table(route_of_channel if sets is None else sets)
        nch = table.size if nr_channels is None else nr_channels
        flags |= MFM_RUNROUTE_F_PACK if pack else 0
        cfg = RunRouteConfig(abi_version, device, nch, nr_routes, window_samples, max_windows, max_runs, max_in_samples, preroll_windows, flags)
        create = "mfm_runroute_create" if sets is None else "mfm_runroute_create_local" if local else "mfm_runroute_create_sets"
        rc = getattr(self.lib, create)(C.byref(self.h), C.byref(cfg), ptr)
        if rc < 0:
            self._raise(rc, create)
        self.nr_channels = nch
        self.nr_routes = nr_routes
        self.pack = bool(flags & MFM_RUNROUTE_F_PACK)
        self.local = bool(local)

    @classmethod
    def behind(cls, route_of_channel, nr_routes, max_in_samples, window_samples, preroll_windows=0, max_open_windows=0, device=0, sets=None,
               pack=False, local=False):
        """a router sized for everything one call of a Gate made from these numbers can hand over (its max_in_samples,
        window_samples, preroll_windows and max_open_windows): the capacity a RunResampler made from them has"""
        return cls(route_of_channel, nr_routes, window_samples=window_samples, max_in_samples=max_in_samples,
                   preroll_windows=preroll_windows, max_windows=max_open_windows, device=device, sets=sets, pack=pack, local=local)

    def bound_view(self):
        """local=True only: the device address of one uint64, fixed at create, that every process_device call writes with the gate's
        payload elements (0 for a call refused for the whole router): RunResampler.process_view_device's d_payload_elems"""
        p = C.c_void_p()
        rc = self.lib.mfm_runroute_bound_view(self.h, C.byref(p))
        if rc < 0:
            self._raise(rc, "mfm_runroute_bound_view")
        return p.value

    def route_channels(self, route):
        """the global channel numbers of one route, ascending (uint32): under pack, local channel i is element i"""
        out = np.zeros(max(self.nr_channels, 1), np.uint32)
        nr = C.c_size_t()
        rc = self.lib.mfm_runroute_route_channels(self.h, route, out.ctypes.data, self.nr_channels, C.byref(nr))
        if rc < 0:
            self._raise(rc, "mfm_runroute_route_channels")
        return out[:nr.value].copy()

    def route_caps(self, route):
        """(nr_channels, max_windows, max_runs) to make one route's RunResampler with: the whole gate's without pack (max_windows
        as given to the router, 0 = the resampler's default), the route's own under pack"""
        n, w, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.lib.mfm_runroute_route_caps(self.h, route, C.byref(n), C.byref(w), C.byref(r))
        if rc < 0:
            self._raise(rc, "mfm_runroute_route_caps")
        return n.value, w.value, r.value

    def fetch_payload(self, route, max_elems=None):
        """pack only: one route's dense int16 payload of the last call.  With max_elems too small: MfmError(MFM_E_NOMEM) whose
        `needed` attribute is the elements that would fit"""
        ne = C.c_size_t()
        if max_elems is None:
            rc = self.lib.mfm_runroute_fetch_payload(self.h, route, None, 0, C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below
                self._raise(rc, "mfm_runroute_fetch_payload")
            max_elems = ne.value
        payload = np.zeros(max(max_elems, 1), np.int16)
        rc = self.lib.mfm_runroute_fetch_payload(self.h, route, payload.ctypes.data, max_elems, C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runroute_fetch_payload")
            except MfmError as err:
                err.needed = ne.value
                raise
        return payload[:ne.value].copy()

    def close(self):
        if self.h:
            self.lib.mfm_runroute_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of Gate.device_view(), after the gate's process_device or flush_device on the same stream"""
        rc = self.lib.mfm_runroute_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals),
                                                  C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runroute_process_device")

    def device_view(self, route):
        """(d_runs, d_payload, d_totals) of one route, for RunResampler.process_device / process_bits_device: its run list, the
        gate's payload pointer and its four uint64 totals (runs, the gate's payload elements, overflow, out of step).  Under local
        the second total is the route's load, and the view goes to process_view_device / process_bits_view_device with bound_view()"""
        r, p, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runroute_device_view(self.h, route, C.byref(r), C.byref(p), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runroute_device_view")
        return r.value, p.value, t.value

    def fetch(self, route, max_runs=None):
        """(runs, nr_elems) of one route of the last call: GATE_RUN_DTYPE [nr_runs] and the gate's payload elements (under pack the
        route's own payload elements, under local the route's load: the samples of its records).  With
        max_runs too small: MfmError(MFM_E_NOMEM) whose `needed` attribute is the runs that would fit"""
        nr, ne = C.c_size_t(), C.c_size_t()
        if max_runs is None:
            rc = self.lib.mfm_runroute_fetch(self.h, route, None, 0, C.byref(nr), C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffer
                self._raise(rc, "mfm_runroute_fetch")
            max_runs = nr.value
        runs = np.zeros(max(max_runs, 1), GATE_RUN_DTYPE)
        rc = self.lib.mfm_runroute_fetch(self.h, route, runs.ctypes.data, max_runs, C.byref(nr), C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runroute_fetch")
            except MfmError as err:
                err.needed = nr.value
                err.buffers = (runs,)
                raise
        return runs[:nr.value].copy(), ne.value

    def capacity(self):
        """max_runs: the most runs one gate call may carry, as given or the RunResampler's default for the same numbers"""
        nr = C.c_uint32()
        rc = self.lib.mfm_runroute_get_capacity(self.h, C.byref(nr))
        if rc < 0:
            self._raise(rc, "mfm_runroute_get_capacity")
        return nr.value


def hosttwin_runroute_capacity(route_of_channel, nr_routes, window_samples=0, max_in_samples=0, preroll_windows=0, max_windows=0,
                               max_runs=0, flags=0, abi_version=MFM_ABI_VERSION, nr_channels=None):
    """mfm_hosttwin_runroute_capacity: what RunRouter(...) with these arguments checks and derives, without a device: the run
    capacity, or MfmError(MFM_E_INVAL) with create's message"""
    lib = load_library()
    table, ptr = _route_table(route_of_channel)
    nch = table.size if nr_channels is None else nr_channels
    cfg = RunRouteConfig(abi_version, 0, nch, nr_routes, window_samples, max_windows, max_runs, max_in_samples, preroll_windows, flags)
    cap = C.c_uint32()
    rc = lib.mfm_hosttwin_runroute_capacity(C.byref(cfg), ptr, C.byref(cap))
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runroute_capacity", lib.mfm_last_error().decode())
    return cap.value


def hosttwin_runroute_call(route_of_channel, nr_routes, gate_runs, gate_totals, max_runs=None, runs=None):
    """mfm_hosttwin_runroute_call: one call of the router on the CPU.  gate_runs GATE_RUN_DTYPE [n], gate_totals the gate's four
    uint64; max_runs the router's capacity (default: len(gate_runs)).  Returns (runs, totals): GATE_RUN_DTYPE [nr_routes][max_runs]
    (`runs` given: written in place; the used part of row k is totals[k][0] long) and uint64 [nr_routes][4]"""
    lib = load_library()
    table, ptr = _route_table(route_of_channel)
    gr = np.ascontiguousarray(gate_runs, dtype=GATE_RUN_DTYPE)
    gt = np.ascontiguousarray(gate_totals, dtype=np.uint64)
    assert gt.shape == (4,)
    max_runs = len(gr) if max_runs is None else max_runs
    if runs is None:
        runs = np.zeros((max(nr_routes, 1), max(max_runs, 1)), GATE_RUN_DTYPE)
    assert runs.dtype == GATE_RUN_DTYPE and runs.flags.c_contiguous and runs.shape[1] == max(max_runs, 1)
    totals = np.zeros((max(nr_routes, 1), 4), np.uint64)
    stride = runs.shape[1]   # rows are max(max_runs, 1) apart: with max_runs 0 nothing is written
    rc = lib.mfm_hosttwin_runroute_call(table.size, nr_routes, ptr, stride if max_runs else 0, gr.ctypes.data if gr.size else None,
                                        gt.ctypes.data, runs.ctypes.data, totals.ctypes.data)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runroute_call", lib.mfm_last_error().decode() or lib.mfm_strerror(rc).decode())
    return runs, totals[:nr_routes]


def hosttwin_runroute_route_caps(sets, nr_routes, route, window_samples=0, max_in_samples=0, preroll_windows=0, max_windows=0, max_runs=0,
                                 pack=False, flags=0, abi_version=MFM_ABI_VERSION, nr_channels=None):
    """mfm_hosttwin_runroute_route_caps: what RunRouter(sets=..., pack=...) with these arguments checks, and what its
    route_caps(route) then returns, without a device: (nr_channels, max_windows, max_runs), or MfmError(MFM_E_INVAL) with create's
    message"""
    lib = load_library()
    table, ptr = _route_table(sets)
    nch = table.size if nr_channels is None else nr_channels
    flags |= MFM_RUNROUTE_F_PACK if pack else 0
    cfg = RunRouteConfig(abi_version, 0, nch, nr_routes, window_samples, max_windows, max_runs, max_in_samples, preroll_windows, flags)
    n, w, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib.mfm_hosttwin_runroute_route_caps(C.byref(cfg), ptr, route, C.byref(n), C.byref(w), C.byref(r))
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runroute_route_caps", lib.mfm_last_error().decode())
    return n.value, w.value, r.value


def hosttwin_runroute_sets_call(sets, nr_routes, gate_runs, gate_totals, max_runs=None, pack=False, window_samples=0, gate_payload=None,
                                route_max_runs=None, route_max_windows=None, flags=0):
    """mfm_hosttwin_runroute_sets_call: one call of a router made with sets= on the CPU.  As hosttwin_runroute_call; under pack
    gate_payload is the gate's int16 payload of gate_totals[1] elements and route_max_runs / route_max_windows are the routes' own
    capacities (default: no limit below the call's own runs and windows).  Returns (runs, totals) and under pack (runs, totals,
    payloads): payloads int16 [nr_routes][max_elems], the used part of row k is totals[k][1] long"""
    lib = load_library()
    table, ptr = _route_table(sets)
    gr = np.ascontiguousarray(gate_runs, dtype=GATE_RUN_DTYPE)
    gt = np.ascontiguousarray(gate_totals, dtype=np.uint64)
    assert gt.shape == (4,)
    max_runs = len(gr) if max_runs is None else max_runs
    flags |= MFM_RUNROUTE_F_PACK if pack else 0
    K = max(nr_routes, 1)
    runs = np.zeros((K, max(max_runs, 1)), GATE_RUN_DTYPE)
    totals = np.zeros((K, 4), np.uint64)
    stride = runs.shape[1] if max_runs else 0
    rmr = rmw = gp = payloads = None
    max_elems = 0
    if flags & MFM_RUNROUTE_F_PACK:
        all_windows = int(gr["nr_windows"].astype(np.uint64).sum())
        rmr = np.ascontiguousarray(np.full(K, max_runs) if route_max_runs is None else route_max_runs, dtype=np.uint32)
        rmw = np.ascontiguousarray(np.full(K, all_windows) if route_max_windows is None else route_max_windows, dtype=np.uint32)
        assert rmr.shape == rmw.shape == (K,)
        gp = np.ascontiguousarray(np.zeros(0, np.int16) if gate_payload is None else gate_payload, dtype=np.int16).reshape(-1)
        assert gp.size >= int(gt[1]), "gate_payload is shorter than gate_totals[1]"
        max_elems = max(int(rmw.max()) * window_samples, 1)
        payloads = np.zeros((K, max_elems), np.int16)
    rc = lib.mfm_hosttwin_runroute_sets_call(table.size, nr_routes, ptr, flags, window_samples, stride, rmr.ctypes.data if rmr is not None else None,
                                             rmw.ctypes.data if rmw is not None else None, gr.ctypes.data if gr.size else None,
                                             gp.ctypes.data if gp is not None and gp.size else None, gt.ctypes.data, runs.ctypes.data,
                                             totals.ctypes.data, payloads.ctypes.data if payloads is not None else None, max_elems)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runroute_sets_call", lib.mfm_last_error().decode() or lib.mfm_strerror(rc).decode())
    if flags & MFM_RUNROUTE_F_PACK:
        return runs, totals[:nr_routes], payloads
    return runs, totals[:nr_routes]


def hosttwin_runroute_local_call(sets, nr_routes, gate_runs, gate_totals, window_samples, max_runs=None, route_max_runs=None,
                                 route_max_windows=None):
    """mfm_hosttwin_runroute_local_call: one call of a router made with sets= and local=True on the CPU.  As
    hosttwin_runroute_sets_call under pack without the payloads: route_max_runs / route_max_windows are the routes' own capacities
    (default: no limit below the call's own runs and windows).  Returns (runs, totals, payload_elems): GATE_RUN_DTYPE
    [nr_routes][max_runs] with route-local channel numbers and the gate's payload offsets, uint64 [nr_routes][4] whose [k][1] is
    the route's load, and what the call leaves behind RunRouter.bound_view()"""
    lib = load_library()
    table, ptr = _route_table(sets)
    gr = np.ascontiguousarray(gate_runs, dtype=GATE_RUN_DTYPE)
    gt = np.ascontiguousarray(gate_totals, dtype=np.uint64)
    assert gt.shape == (4,)
    max_runs = len(gr) if max_runs is None else max_runs
    K = max(nr_routes, 1)
    runs = np.zeros((K, max(max_runs, 1)), GATE_RUN_DTYPE)
    totals = np.zeros((K, 4), np.uint64)
    stride = runs.shape[1] if max_runs else 0
    all_windows = int(gr["nr_windows"].astype(np.uint64).sum())
    rmr = np.ascontiguousarray(np.full(K, max_runs) if route_max_runs is None else route_max_runs, dtype=np.uint32)
    rmw = np.ascontiguousarray(np.full(K, all_windows) if route_max_windows is None else route_max_windows, dtype=np.uint32)
    assert rmr.shape == rmw.shape == (K,)
    bound = C.c_uint64()
    rc = lib.mfm_hosttwin_runroute_local_call(table.size, nr_routes, ptr, window_samples, stride, rmr.ctypes.data, rmw.ctypes.data,
                                              gr.ctypes.data if gr.size else None, gt.ctypes.data, runs.ctypes.data, totals.ctypes.data,
                                              C.byref(bound))
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runroute_local_call", lib.mfm_last_error().decode() or lib.mfm_strerror(rc).decode())
    return runs, totals[:nr_routes], bound.value


# numpy views of the stretch-end records: struct mfm_runais_end (48 bytes), mfm_runpocsag_end (184), mfm_runflex_end (64)
RUNAIS_END_DTYPE = np.dtype([("stretch_window", "<u8"), ("outs", "<u8"), ("start_sample", "<u8"), ("channel", "<u4"), ("run", "<u4"),
                             ("mode", "<u4"), ("nr_bits", "<u4"), ("reserved", "<u4", (2,))])
RUNPOCSAG_END_DTYPE = np.dtype([("stretch_window", "<u8"), ("outs", "<u8"), ("channel", "<u4"), ("run", "<u4"), ("mode", "<u4"),
                                ("baud", "<u4"), ("nr_words", "<u4"), ("nr_bits", "<u4"), ("nr_sync_bits", "<u4"), ("reserved", "<u4"),
                                ("nr_ok", "<u4"), ("fail_mask", "<u4"), ("raw", "<u4", (16,)), ("corrected", "<u4", (16,))])
RUNFLEX_END_DTYPE = np.dtype([("stretch_window", "<u8"), ("outs", "<u8"), ("j", "<u8"), ("channel", "<u4"), ("run", "<u4"),
                              ("mode", "<u4"), ("eye", "<u4"), ("coding", "<u4"), ("fiw", "<u4"), ("cycle", "<u4"), ("frame", "<u4"),
                              ("reserved", "<u4", (2,))])
assert (RUNAIS_END_DTYPE.itemsize, RUNPOCSAG_END_DTYPE.itemsize, RUNFLEX_END_DTYPE.itemsize) == (48, 184, 64)
RUN_ENDS_NO_RUN = 0xffffffff   # `run` of a record the end call wrote


class _RunEnds:
    """the stretch-end report of a burst stage (mfm_<stage>_set_end_report and kin): one record per stretch that says how it
    ended and what the closing squelch cut.  Off at create."""
    _ends_stage = None   # "runais" / "runpocsag" / "runflex"
    _ends_dtype = None

    def _ends_fn(self, what):
        return getattr(self.lib, f"mfm_{self._ends_stage}_{what}"), f"mfm_{self._ends_stage}_{what}"

    def set_end_report(self, on=True):
        """valid only before the first process call: MfmError(MFM_E_STATE) afterwards"""
        fn, name = self._ends_fn("set_end_report")
        rc = fn(self.h, 1 if on else 0)
        if rc < 0:
            self._raise(rc, name)

    def end_stretches(self, stream=None):
        """the end of a stream, behind the gate's flush: a record for every channel with a stretch, then no channel has one"""
        fn, name = self._ends_fn("end_stretches_device")
        rc = fn(self.h, C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, name)

    def fetch_ends(self, max_ends=None):
        """the records of the last call, process or end (a structured array of the stage's END dtype).  With max_ends too small:
        MfmError(MFM_E_NOMEM) whose `needed` attribute is the number that would fit"""
        fn, name = self._ends_fn("fetch_ends")
        nr = C.c_size_t()
        if max_ends is None:
            rc = fn(self.h, None, 0, C.byref(nr))
            if rc not in (MFM_OK, MFM_E_NOMEM):
                self._raise(rc, name)
            max_ends = nr.value
        out = np.zeros(max(max_ends, 1), self._ends_dtype)
        rc = fn(self.h, out.ctypes.data, max_ends, C.byref(nr))
        if rc < 0:
            try:
                self._raise(rc, name)
            except MfmError as err:
                err.needed = nr.value
                err.buffer = out
                raise
        return out[:nr.value].copy()

    def ends_view(self):
        """(d_ends, d_end_totals): device addresses of the last call's records and of { records, records with mode != 0 }"""
        fn, name = self._ends_fn("ends_view")
        e, t = C.c_void_p(), C.c_void_p()
        rc = fn(self.h, C.byref(e), C.byref(t))
        if rc < 0:
            self._raise(rc, name)
        return e.value, t.value


def _twin_ends_error(lib, rc, what, **attrs):
    err = MfmError(rc, what, lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
    for k, v in attrs.items():
        setattr(err, k, v)
    return err


def _twin_call_args(runs, payload, totals, max_runs, max_out_samples):
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(payload, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, pl.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    return rr, pl, t, (max(rr.size, 1) if max_runs is None else max_runs), (max(pl.size, 1) if max_out_samples is None else max_out_samples)


def hosttwin_runais_call_ends(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_out=None,
                              max_ends=None):
    """mfm_hosttwin_runais_call_ends: hosttwin_runais_call with the stretch-end records of the call; returns (events, ends).
    max_ends too small: MfmError(MFM_E_NOMEM) with `needed_ends`, nothing written"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNAIS_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr, pl, t, max_runs, max_out_samples = _twin_call_args(runs, payload, totals, max_runs, max_out_samples)
    max_out = pl.size // 160 + rr.size if max_out is None else max_out
    max_ends = rr.size if max_ends is None else max_ends
    out, ends = np.zeros(max(max_out, 1), RUNAIS_EVENT_DTYPE), np.zeros(max(max_ends, 1), RUNAIS_END_DTYPE)
    nr, fl, ne = C.c_size_t(), C.c_uint32(), C.c_size_t()
    rc = lib.mfm_hosttwin_runais_call_ends(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                           rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                           out.ctypes.data, max_out, C.byref(nr), C.byref(fl), ends.ctypes.data, max_ends, C.byref(ne))
    if rc < 0:
        raise _twin_ends_error(lib, rc, "mfm_hosttwin_runais_call_ends", needed=nr.value, flags=fl.value, needed_ends=ne.value)
    return out[:nr.value].copy(), ends[:ne.value].copy()


def hosttwin_runpocsag_call_ends(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_out=None,
                                 max_ends=None):
    """mfm_hosttwin_runpocsag_call_ends: hosttwin_runpocsag_call with the stretch-end records of the call; returns (events, ends)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNPOCSAG_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr, pl, t, max_runs, max_out_samples = _twin_call_args(runs, payload, totals, max_runs, max_out_samples)
    max_out = int(sum(runpocsag_slots(int(n)) for n in rr["nr_out"])) if max_out is None else max_out
    max_ends = rr.size if max_ends is None else max_ends
    out, ends = np.zeros(max(max_out, 1), RUNPOCSAG_EVENT_DTYPE), np.zeros(max(max_ends, 1), RUNPOCSAG_END_DTYPE)
    nr, fl, ne = C.c_size_t(), C.c_uint32(), C.c_size_t()
    rc = lib.mfm_hosttwin_runpocsag_call_ends(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                              rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                              out.ctypes.data, max_out, C.byref(nr), C.byref(fl), ends.ctypes.data, max_ends, C.byref(ne))
    if rc < 0:
        raise _twin_ends_error(lib, rc, "mfm_hosttwin_runpocsag_call_ends", needed=nr.value, flags=fl.value, needed_ends=ne.value)
    return out[:nr.value].copy(), ends[:ne.value].copy()


def hosttwin_runflex_call_ends(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_frames=0,
                               max_out=None, max_out_frames=None, max_ends=None):
    """mfm_hosttwin_runflex_call_ends: hosttwin_runflex_call with the stretch-end records of the call; returns (events, frames,
    ends)"""
    lib = load_library()
    st, ring = state
    assert st.dtype == RUNFLEX_STATE_DTYPE and st.flags.c_contiguous and st.ndim == 1
    assert ring.dtype == np.int16 and ring.flags.c_contiguous and ring.shape == (st.shape[0], RUNFLEX_RING)
    rr, pl, t, max_runs, max_out_samples = _twin_call_args(runs, payload, totals, max_runs, max_out_samples)
    max_out = pl.size // RUNFLEX_EVENT_SPACING + rr.size if max_out is None else max_out
    max_out_frames = pl.size // RUNFLEX_FRAME_SPACING + rr.size if max_out_frames is None else max_out_frames
    max_ends = rr.size if max_ends is None else max_ends
    ev, fw = np.zeros(max(max_out, 1), RUNFLEX_EVENT_DTYPE), np.zeros(max(max_out_frames, 1), FLEX_FRAME_DTYPE)
    ends = np.zeros(max(max_ends, 1), RUNFLEX_END_DTYPE)
    nev, nf, fl, ne = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_size_t()
    rc = lib.mfm_hosttwin_runflex_call_ends(st.shape[0], max_runs, max_out_samples, max_events, max_frames, st.ctypes.data, ring.ctypes.data,
                                            rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                            ev.ctypes.data, max_out, C.byref(nev), fw.ctypes.data, max_out_frames, C.byref(nf), C.byref(fl),
                                            ends.ctypes.data, max_ends, C.byref(ne))
    if rc < 0:
        raise _twin_ends_error(lib, rc, "mfm_hosttwin_runflex_call_ends", needed=nev.value, needed_frames=nf.value, flags=fl.value,
                               needed_ends=ne.value)
    return ev[:nev.value].copy(), fw[:nf.value].copy(), ends[:ne.value].copy()


def _twin_end_stretches(name, st, dtype, end_dtype, max_ends):
    lib = load_library()
    assert st.dtype == dtype and st.flags.c_contiguous and st.ndim == 1
    max_ends = st.shape[0] if max_ends is None else max_ends
    ends, ne = np.zeros(max(max_ends, 1), end_dtype), C.c_size_t()
    rc = getattr(lib, name)(st.shape[0], st.ctypes.data, ends.ctypes.data, max_ends, C.byref(ne))
    if rc < 0:
        raise _twin_ends_error(lib, rc, name, needed_ends=ne.value)
    return ends[:ne.value].copy()


def hosttwin_runais_end_stretches(state, max_ends=None):
    """mfm_hosttwin_runais_end_stretches: the end call on the CPU; returns the records, state is all zero afterwards"""
    return _twin_end_stretches("mfm_hosttwin_runais_end_stretches", np.asarray(state), RUNAIS_STATE_DTYPE, RUNAIS_END_DTYPE, max_ends)


def hosttwin_runpocsag_end_stretches(state, max_ends=None):
    """mfm_hosttwin_runpocsag_end_stretches: the end call on the CPU; returns the records, state is all zero afterwards"""
    return _twin_end_stretches("mfm_hosttwin_runpocsag_end_stretches", np.asarray(state), RUNPOCSAG_STATE_DTYPE, RUNPOCSAG_END_DTYPE, max_ends)


def hosttwin_runflex_end_stretches(state, max_ends=None):
    """mfm_hosttwin_runflex_end_stretches: the end call on the CPU; state = (state, ring), the ring is not touched"""
    return _twin_end_stretches("mfm_hosttwin_runflex_end_stretches", state[0], RUNFLEX_STATE_DTYPE, RUNFLEX_END_DTYPE, max_ends)


class RunAis(_RunEnds):
    """mfm_runais: the runs of a RunResampler's device view through the AIS demodulator, one fresh demodulator per stretch;
    one RUNAIS_EVENT_DTYPE per candidate packet.  max_runs and max_out_samples are the burst resampler's capacities
    (RunAis.behind reads them); max_events 0 is a bound that cannot overflow."""
    _ends_stage, _ends_dtype = "runais", RUNAIS_END_DTYPE

    def __init__(self, nr_channels, max_runs, max_out_samples, max_events=0, device=0, flags=0, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = RunaisConfig(abi_version, device, nr_channels, max_runs, max_out_samples, max_events, flags)
        rc = self.lib.mfm_runais_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            self._raise(rc, "mfm_runais_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_resampler, max_events=0, device=0):
        """a stage sized for everything one call of `run_resampler` can produce"""
        max_runs, max_out = run_resampler.capacity()
        return cls(run_resampler.nr_channels, max_runs, max_out, max_events=max_events, device=device)

    def close(self):
        if self.h:
            self.lib.mfm_runais_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of RunResampler.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runais_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runais_process_device")

    def process_bits_device(self, view, stream=None):
        """as process_device, from a RunResampler's MFM_BITS_POS bits_view() instead of PCM"""
        rc = self.lib.mfm_runais_process_bits_device(self.h, C.byref(view), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runais_process_bits_device")

    def fetch(self, max_events=None):
        """the events of the last call (RUNAIS_EVENT_DTYPE).  With max_events too small: MfmError(MFM_E_NOMEM) whose `needed`
        attribute is the number that would fit and whose `buffer` is untouched"""
        nr = C.c_size_t()
        if max_events is None:
            rc = self.lib.mfm_runais_fetch(self.h, None, 0, C.byref(nr))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffer
                self._raise(rc, "mfm_runais_fetch")
            max_events = nr.value
        out = np.zeros(max(max_events, 1), RUNAIS_EVENT_DTYPE)
        rc = self.lib.mfm_runais_fetch(self.h, out.ctypes.data, max_events, C.byref(nr))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runais_fetch")
            except MfmError as err:
                err.needed = nr.value
                err.buffer = out
                raise
        return out[:nr.value].copy()

    def device_view(self):
        """(d_events, d_totals): device addresses of the last call's events and the four uint64 totals (events, runs, overflow,
        input error)"""
        e, t = C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runais_device_view(self.h, C.byref(e), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runais_device_view")
        return e.value, t.value

    def fetch_state(self):
        """the per-channel state the last call left (RUNAIS_STATE_DTYPE [C]): what the host twin carries"""
        out = np.zeros(self.nr_channels, RUNAIS_STATE_DTYPE)
        rc = self.lib.mfm_runais_fetch_state(self.h, out.ctypes.data, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runais_fetch_state")
        return out

    def store_state(self, state, nr_channels=None):
        """mfm_runais_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNAIS_STATE_DTYPE) if state is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        rc = self.lib.mfm_runais_store_state(self.h, st.ctypes.data if st is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runais_store_state")


def hosttwin_runais_state(nr_channels):
    """the host twin's per-channel state at the start of a stream: RUNAIS_STATE_DTYPE [C], all zero (no stretch)"""
    return np.zeros(nr_channels, RUNAIS_STATE_DTYPE)


def hosttwin_runais_call(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_out=None):
    """mfm_hosttwin_runais_call: one call of the burst AIS stage on the CPU.  state (hosttwin_runais_state) is updated in
    place; runs RUNRS_RUN_DTYPE and payload int16 are one burst resampler call's result, totals its four totals (default: the
    lengths, no flags); max_runs / max_out_samples / max_events are the configuration's (default: what the call needs);
    returns the events.  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute (overflow | input error << 8)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNAIS_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(payload, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, pl.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(pl.size, 1) if max_out_samples is None else max_out_samples
    if max_out is None:
        max_out = pl.size // 160 + rr.size
    out = np.zeros(max(max_out, 1), RUNAIS_EVENT_DTYPE)
    nr, fl = C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runais_call(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                      rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                      out.ctypes.data, max_out, C.byref(nr), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runais_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = nr.value, fl.value
        raise err
    return out[:nr.value].copy()


def hosttwin_runais_call_bits(state, runs, bits, polarity=MFM_BITS_POS, totals=None, max_runs=None, max_out_samples=None, max_events=0,
                              max_out=None):
    """mfm_hosttwin_runais_call_bits: hosttwin_runais_call on the burst resampler's bits form.  runs (out_offset in words)
    and bits uint32 are one bits call's result, totals its four totals (default: the lengths, no flags); the same state may go
    through PCM and bits calls in turn"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNAIS_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    bw = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    t = np.array([rr.size, bw.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    nout = int(rr["nr_out"].astype(np.uint64).sum())
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(nout, 1) if max_out_samples is None else max_out_samples
    if max_out is None:
        max_out = nout // 160 + rr.size
    out = np.zeros(max(max_out, 1), RUNAIS_EVENT_DTYPE)
    nr, fl = C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runais_call_bits(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                           rr.ctypes.data if rr.size else None, bw.ctypes.data if bw.size else None, polarity,
                                           t.ctypes.data, out.ctypes.data, max_out, C.byref(nr), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runais_call_bits", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = nr.value, fl.value
        raise err
    return out[:nr.value].copy()


def runais_to_ais_events(events, interpolate, decimate, window_samples):
    """mfm_ais_event records (AIS_EVENT_DTYPE, what host/mfm_ais.c's ais_decode_on_events takes) from the burst stage's: the
    stretch-relative sample numbers become positions of the channel's stream at the output rate, sample = stretch_window * W *
    I // D + sample and start_sample likewise.  That is the position to within one sample: a fresh resampler's first output
    stands for the stretch's first input sample, and the floor drops less than one output period"""
    ev = np.asarray(events)
    assert ev.dtype == RUNAIS_EVENT_DTYPE
    out = np.zeros(ev.shape, AIS_EVENT_DTYPE)
    base = np.array([int(w) * window_samples * interpolate // decimate for w in ev["stretch_window"]], np.uint64).reshape(ev.shape)
    for f in ("channel", "fcs_valid", "nr_bytes", "bytes"):
        out[f] = ev[f]
    out["sample"] = base + ev["sample"]
    out["start_sample"] = base + ev["start_sample"]
    return out


class RunPocsag(_RunEnds):
    """mfm_runpocsag: the runs of a RunResampler's device view (38 400 Hz) through the POCSAG demodulator, one fresh demodulator
    per stretch; RUNPOCSAG_EVENT_DTYPE records.  max_runs and max_out_samples are the burst resampler's capacities
    (RunPocsag.behind reads them); max_events 0 is a bound that cannot overflow."""
    _ends_stage, _ends_dtype = "runpocsag", RUNPOCSAG_END_DTYPE

    def __init__(self, nr_channels, max_runs, max_out_samples, max_events=0, device=0, flags=0, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = RunPocsagConfig(abi_version, device, nr_channels, max_runs, max_out_samples, max_events, flags)
        rc = self.lib.mfm_runpocsag_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_resampler, max_events=0, device=0):
        """a stage sized for everything one call of `run_resampler` can produce"""
        max_runs, max_out = run_resampler.capacity()
        return cls(run_resampler.nr_channels, max_runs, max_out, max_events=max_events, device=device)

    def close(self):
        if self.h:
            self.lib.mfm_runpocsag_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of RunResampler.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runpocsag_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_process_device")

    def process_bits_device(self, view, stream=None):
        """as process_device, from a RunResampler's MFM_BITS_NEG bits_view() instead of PCM"""
        rc = self.lib.mfm_runpocsag_process_bits_device(self.h, C.byref(view), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_process_bits_device")

    def fetch(self, max_events=None):
        """the events of the last call (RUNPOCSAG_EVENT_DTYPE).  With max_events too small: MfmError(MFM_E_NOMEM) whose `needed`
        attribute is the number that would fit and whose `buffer` is untouched"""
        nr = C.c_size_t()
        if max_events is None:
            rc = self.lib.mfm_runpocsag_fetch(self.h, None, 0, C.byref(nr))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffer
                self._raise(rc, "mfm_runpocsag_fetch")
            max_events = nr.value
        out = np.zeros(max(max_events, 1), RUNPOCSAG_EVENT_DTYPE)
        rc = self.lib.mfm_runpocsag_fetch(self.h, out.ctypes.data, max_events, C.byref(nr))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runpocsag_fetch")
            except MfmError as err:
                err.needed = nr.value
                err.buffer = out
                raise
        return out[:nr.value].copy()

    def device_view(self):
        """(d_events, d_totals): device addresses of the last call's events and the four uint64 totals (events, runs, overflow,
        input error)"""
        e, t = C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runpocsag_device_view(self.h, C.byref(e), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_device_view")
        return e.value, t.value

    def fetch_state(self):
        """the per-channel state the last call left (RUNPOCSAG_STATE_DTYPE [C]): what the host twin carries"""
        out = np.zeros(self.nr_channels, RUNPOCSAG_STATE_DTYPE)
        rc = self.lib.mfm_runpocsag_fetch_state(self.h, out.ctypes.data, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_fetch_state")
        return out

    def store_state(self, state, nr_channels=None):
        """mfm_runpocsag_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNPOCSAG_STATE_DTYPE) if state is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        rc = self.lib.mfm_runpocsag_store_state(self.h, st.ctypes.data if st is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runpocsag_store_state")


class RunMm:
    """mfm_runmm: the runs of a RunResampler's device view through the Mueller-Muller clock recovery, one fresh loop per stretch;
    RUNMM_RUN_DTYPE records and a dense int16 payload of decisions.  max_runs and max_out_samples are the burst resampler's
    capacities (RunMm.behind reads them); max_decisions 0 is a bound that cannot overflow.  error_min / error_max default to
    samples_per_bit -/+ margin in float32, as the reference's test sets them."""

    def __init__(self, nr_channels, max_runs, max_out_samples, samples_per_bit, kw, km, margin=0.05, error_min=None, error_max=None,
                 max_decisions=0, device=0, flags=0, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        emin = float(np.float32(samples_per_bit) - np.float32(margin)) if error_min is None else error_min
        emax = float(np.float32(samples_per_bit) + np.float32(margin)) if error_max is None else error_max
        self.cfg = RunMmConfig(abi_version, device, nr_channels, max_runs, max_out_samples, max_decisions, flags, kw, km, samples_per_bit,
                               emin, emax)
        rc = self.lib.mfm_runmm_create(C.byref(self.h), C.byref(self.cfg))
        if rc < 0:
            self._raise(rc, "mfm_runmm_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_resampler, samples_per_bit, kw, km, margin=0.05, max_decisions=0, device=0, **kwargs):
        """a stage sized for everything one call of `run_resampler` can produce"""
        max_runs, max_out = run_resampler.capacity()
        return cls(run_resampler.nr_channels, max_runs, max_out, samples_per_bit, kw, km, margin=margin, max_decisions=max_decisions,
                   device=device, **kwargs)

    def close(self):
        if self.h:
            self.lib.mfm_runmm_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of RunResampler.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runmm_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runmm_process_device")

    def fetch(self, max_runs=None, max_decisions=None):
        """(runs RUNMM_RUN_DTYPE, decisions int16) of the last call.  With a buffer too small: MfmError(MFM_E_NOMEM) whose `needed`
        attribute is the (runs, decisions) that would fit"""
        nr, nd = C.c_size_t(), C.c_size_t()
        if max_runs is None or max_decisions is None:
            rc = self.lib.mfm_runmm_fetch(self.h, None, 0, C.byref(nr), None, 0, C.byref(nd))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below
                self._raise(rc, "mfm_runmm_fetch")
            max_runs = nr.value if max_runs is None else max_runs
            max_decisions = nd.value if max_decisions is None else max_decisions
        runs = np.zeros(max(max_runs, 1), RUNMM_RUN_DTYPE)
        decs = np.zeros(max(max_decisions, 1), np.int16)
        rc = self.lib.mfm_runmm_fetch(self.h, runs.ctypes.data, max_runs, C.byref(nr), decs.ctypes.data, max_decisions, C.byref(nd))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runmm_fetch")
            except MfmError as err:
                err.needed = (nr.value, nd.value)
                raise
        return runs[:nr.value].copy(), decs[:nd.value].copy()

    def device_view(self):
        """(d_runs, d_decisions, d_totals): device addresses of the last call's run records, its decisions and the four uint64
        totals (runs, decisions, overflow, input error)"""
        r, d, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runmm_device_view(self.h, C.byref(r), C.byref(d), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runmm_device_view")
        return r.value, d.value, t.value

    def capacity(self):
        """(max_runs, max_decisions) fixed at create, the default filled in: what a stage behind this one sizes itself from"""
        r, d = C.c_uint32(), C.c_uint64()
        rc = self.lib.mfm_runmm_get_capacity(self.h, C.byref(r), C.byref(d))
        if rc < 0:
            self._raise(rc, "mfm_runmm_get_capacity")
        return r.value, d.value

    def fetch_state(self):
        """the per-channel state the last call left (RUNMM_STATE_DTYPE [C]): what the host twin carries"""
        out = np.zeros(self.nr_channels, RUNMM_STATE_DTYPE)
        rc = self.lib.mfm_runmm_fetch_state(self.h, out.ctypes.data, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runmm_fetch_state")
        return out

    def store_state(self, state, nr_channels=None):
        """mfm_runmm_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNMM_STATE_DTYPE) if state is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        rc = self.lib.mfm_runmm_store_state(self.h, st.ctypes.data if st is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runmm_store_state")


def hosttwin_runmm_state(nr_channels):
    """the host twin's per-channel state at the start of a stream: RUNMM_STATE_DTYPE [C], all zero (no stretch)"""
    return np.zeros(nr_channels, RUNMM_STATE_DTYPE)


def hosttwin_runmm_call(state, runs, payload, samples_per_bit, kw, km, margin=0.05, error_min=None, error_max=None, totals=None,
                        max_runs=None, max_out_samples=None, max_decisions=0, max_out_runs=None, max_out_decisions=None, flags=0,
                        abi_version=MFM_ABI_VERSION):
    """mfm_hosttwin_runmm_call: one call of the burst Mueller-Muller stage on the CPU.  state (hosttwin_runmm_state) is updated in
    place; runs RUNRS_RUN_DTYPE and payload int16 are one burst resampler call's result, totals its four totals (default: the
    lengths, no flags); max_runs / max_out_samples / max_decisions are the configuration's (default: what the call needs);
    returns (runs RUNMM_RUN_DTYPE, decisions).  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute (overflow |
    input error << 8)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNMM_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(payload, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, pl.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(pl.size, 1) if max_out_samples is None else max_out_samples
    emin = float(np.float32(samples_per_bit) - np.float32(margin)) if error_min is None else error_min
    emax = float(np.float32(samples_per_bit) + np.float32(margin)) if error_max is None else error_max
    cfg = RunMmConfig(abi_version, 0, state.shape[0], max_runs, max_out_samples, max_decisions, flags, kw, km, samples_per_bit, emin, emax)
    max_out_runs = rr.size if max_out_runs is None else max_out_runs
    max_out_decisions = pl.size + rr.size if max_out_decisions is None else max_out_decisions
    out_r = np.zeros(max(max_out_runs, 1), RUNMM_RUN_DTYPE)
    out_d = np.zeros(max(max_out_decisions, 1), np.int16)
    nr, nd, fl = C.c_size_t(), C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runmm_call(C.byref(cfg), state.ctypes.data, rr.ctypes.data if rr.size else None,
                                     pl.ctypes.data if pl.size else None, t.ctypes.data, out_r.ctypes.data, max_out_runs, C.byref(nr),
                                     out_d.ctypes.data, max_out_decisions, C.byref(nd), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runmm_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = (nr.value, nd.value), fl.value
        raise err
    return out_r[:nr.value].copy(), out_d[:nd.value].copy()


def hosttwin_runmm_state_check(state):
    """mfm_hosttwin_runmm_state_check: what RunMm.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNMM_STATE_DTYPE).reshape(-1)
    lib = load_library()
    rc = lib.mfm_hosttwin_runmm_state_check(st.shape[0], st.ctypes.data)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runmm_state_check", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())


def _runsync_config(nr_channels, max_runs, max_decisions, words, max_distance, bit_rule, either, max_events, device, flags, abi_version):
    ws = [int(w) & 0xFFFFFFFF for w in words]
    arr = (C.c_uint32 * 8)(*ws[:8])
    fl = (MFM_RUNSYNC_F_EITHER if either else 0) if flags is None else flags
    return RunSyncConfig(abi_version, device, nr_channels, max_runs, max_decisions, max_events, len(ws), arr, max_distance, bit_rule, fl)


class RunSync:
    """mfm_runsync: the decisions of a RunMm's device view against a table of sync words, a fresh 32-bit register per stretch;
    RUNSYNC_RUN_DTYPE records, one bit per decision in words aligned per run, and RUNSYNC_EVENT_DTYPE events.  max_runs and
    max_decisions are the burst Mueller-Muller stage's capacities (RunSync.behind reads them); max_events 0 cannot overflow."""

    def __init__(self, nr_channels, max_runs, max_decisions, words, max_distance=3, bit_rule=MFM_RUNSYNC_BIT_NOT_POS, either=False,
                 max_events=0, device=0, flags=None, abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.cfg = _runsync_config(nr_channels, max_runs, max_decisions, words, max_distance, bit_rule, either, max_events, device, flags,
                                   abi_version)
        rc = self.lib.mfm_runsync_create(C.byref(self.h), C.byref(self.cfg))
        if rc < 0:
            self._raise(rc, "mfm_runsync_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_mm, words, **kwargs):
        """a stage sized for everything one call of `run_mm` can produce"""
        max_runs, max_decisions = run_mm.capacity()
        return cls(run_mm.nr_channels, max_runs, max_decisions, words, **kwargs)

    def close(self):
        if self.h:
            self.lib.mfm_runsync_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_decisions, d_totals, stream=None):
        """the three addresses of RunMm.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runsync_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_decisions), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runsync_process_device")

    def fetch(self, max_runs=None, max_words=None, max_events=None):
        """(runs RUNSYNC_RUN_DTYPE, bits uint32, events RUNSYNC_EVENT_DTYPE) of the last call.  With a buffer too small:
        MfmError(MFM_E_NOMEM) whose `needed` attribute is the (runs, words, events) that would fit"""
        nr, nw, ne = C.c_size_t(), C.c_size_t(), C.c_size_t()
        if max_runs is None or max_words is None or max_events is None:
            rc = self.lib.mfm_runsync_fetch(self.h, None, 0, C.byref(nr), None, 0, C.byref(nw), None, 0, C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below
                self._raise(rc, "mfm_runsync_fetch")
            max_runs = nr.value if max_runs is None else max_runs
            max_words = nw.value if max_words is None else max_words
            max_events = ne.value if max_events is None else max_events
        runs = np.zeros(max(max_runs, 1), RUNSYNC_RUN_DTYPE)
        bits = np.zeros(max(max_words, 1), np.uint32)
        evs = np.zeros(max(max_events, 1), RUNSYNC_EVENT_DTYPE)
        rc = self.lib.mfm_runsync_fetch(self.h, runs.ctypes.data, max_runs, C.byref(nr), bits.ctypes.data, max_words, C.byref(nw),
                                        evs.ctypes.data, max_events, C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runsync_fetch")
            except MfmError as err:
                err.needed = (nr.value, nw.value, ne.value)
                raise
        return runs[:nr.value].copy(), bits[:nw.value].copy(), evs[:ne.value].copy()

    def device_view(self):
        """(d_runs, d_bits, d_events, d_totals): device addresses of the last call's run records, bit words, events and the four
        uint64 totals (runs, events, overflow, input error)"""
        r, b, e, t = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runsync_device_view(self.h, C.byref(r), C.byref(b), C.byref(e), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runsync_device_view")
        return r.value, b.value, e.value, t.value

    def capacity(self):
        """(max_runs, max_words, max_events) fixed at create"""
        r, w, e = C.c_uint32(), C.c_uint64(), C.c_uint64()
        rc = self.lib.mfm_runsync_get_capacity(self.h, C.byref(r), C.byref(w), C.byref(e))
        if rc < 0:
            self._raise(rc, "mfm_runsync_get_capacity")
        return r.value, w.value, e.value

    def fetch_state(self):
        """the per-channel state the last call left (RUNSYNC_STATE_DTYPE [C]): what the host twin carries"""
        out = np.zeros(self.nr_channels, RUNSYNC_STATE_DTYPE)
        rc = self.lib.mfm_runsync_fetch_state(self.h, out.ctypes.data, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runsync_fetch_state")
        return out

    def store_state(self, state, nr_channels=None):
        """mfm_runsync_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNSYNC_STATE_DTYPE) if state is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        rc = self.lib.mfm_runsync_store_state(self.h, st.ctypes.data if st is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runsync_store_state")


def hosttwin_runsync_state(nr_channels):
    """the host twin's per-channel state at the start of a stream: RUNSYNC_STATE_DTYPE [C], all zero (no stretch)"""
    return np.zeros(nr_channels, RUNSYNC_STATE_DTYPE)


def hosttwin_runsync_call(state, runs, decisions, words, max_distance=3, bit_rule=MFM_RUNSYNC_BIT_NOT_POS, either=False, totals=None,
                          max_runs=None, max_decisions=None, max_events=0, max_out_runs=None, max_out_words=None, max_out_events=None,
                          flags=None, abi_version=MFM_ABI_VERSION):
    """mfm_hosttwin_runsync_call: one call of the burst sync stage on the CPU.  state (hosttwin_runsync_state) is updated in place;
    runs RUNMM_RUN_DTYPE and decisions int16 are one burst Mueller-Muller call's result, totals its four totals (default: the
    lengths, no flags); max_runs / max_decisions / max_events are the configuration's (default: what the call needs); returns
    (runs RUNSYNC_RUN_DTYPE, bits, events).  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute (overflow | input
    error << 8)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNSYNC_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNMM_RUN_DTYPE).reshape(-1)
    dd = np.ascontiguousarray(decisions, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, dd.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_decisions = max(dd.size, 1) if max_decisions is None else max_decisions
    cfg = _runsync_config(state.shape[0], max_runs, max_decisions, words, max_distance, bit_rule, either, max_events, 0, flags, abi_version)
    max_out_runs = rr.size if max_out_runs is None else max_out_runs
    max_out_words = dd.size // 32 + rr.size if max_out_words is None else max_out_words
    max_out_events = dd.size if max_out_events is None else max_out_events
    out_r = np.zeros(max(max_out_runs, 1), RUNSYNC_RUN_DTYPE)
    out_b = np.zeros(max(max_out_words, 1), np.uint32)
    out_e = np.zeros(max(max_out_events, 1), RUNSYNC_EVENT_DTYPE)
    nr, nw, ne, fl = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runsync_call(C.byref(cfg), state.ctypes.data, rr.ctypes.data if rr.size else None,
                                       dd.ctypes.data if dd.size else None, t.ctypes.data, out_r.ctypes.data, max_out_runs, C.byref(nr),
                                       out_b.ctypes.data, max_out_words, C.byref(nw), out_e.ctypes.data, max_out_events, C.byref(ne),
                                       C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runsync_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = (nr.value, nw.value, ne.value), fl.value
        raise err
    return out_r[:nr.value].copy(), out_b[:nw.value].copy(), out_e[:ne.value].copy()


def hosttwin_runsync_state_check(state):
    """mfm_hosttwin_runsync_state_check: what RunSync.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNSYNC_STATE_DTYPE).reshape(-1)
    lib = load_library()
    rc = lib.mfm_hosttwin_runsync_state_check(st.shape[0], st.ctypes.data)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runsync_state_check", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())


def _runbatch_config(nr_channels, max_runs, max_decisions, words, word_mask, keep_distance, max_events, device, flags, abi_version):
    ws = [int(w) & 0xFFFFFFFF for w in words]
    arr = (C.c_uint32 * 8)(*ws[:8])
    return RunBatchConfig(abi_version, device, nr_channels, max_runs, max_decisions, max_events, len(ws), arr, word_mask, keep_distance, flags)


class RunBatch:
    """mfm_runbatch: behind the sync events of a RunSync's device view, POCSAG batches of 16 codewords cut from its bit words, BCH
    on them, and sync kept / sync lost in the slot behind every batch (pager/pager_pocsag.c:468-538 at one sample per bit);
    RUNBATCH_EVENT_DTYPE events of the MFM_POCSAG_EV_* types.  max_runs and max_decisions are the burst sync stage's (RunBatch.behind
    reads them), words its table; max_events 0 cannot overflow."""

    def __init__(self, nr_channels, max_runs, max_decisions, words, word_mask=0, keep_distance=4, max_events=0, device=0, flags=0,
                 abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.cfg = _runbatch_config(nr_channels, max_runs, max_decisions, words, word_mask, keep_distance, max_events, device, flags, abi_version)
        rc = self.lib.mfm_runbatch_create(C.byref(self.h), C.byref(self.cfg))
        if rc < 0:
            self._raise(rc, "mfm_runbatch_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_sync, **kwargs):
        """a stage sized for everything one call of `run_sync` can produce, with its table of words"""
        cfg = run_sync.cfg
        return cls(run_sync.nr_channels, cfg.max_runs, cfg.max_decisions, list(cfg.words)[:cfg.nr_words], **kwargs)

    def close(self):
        if self.h:
            self.lib.mfm_runbatch_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_bits, d_events, d_totals, stream=None):
        """the four addresses of RunSync.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runbatch_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_bits), C.c_void_p(d_events), C.c_void_p(d_totals),
                                                  C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runbatch_process_device")

    def fetch(self, max_events=None):
        """the RUNBATCH_EVENT_DTYPE events of the last call.  With a buffer too small: MfmError(MFM_E_NOMEM) whose `needed`
        attribute is the number that would fit"""
        ne = C.c_size_t()
        if max_events is None:
            rc = self.lib.mfm_runbatch_fetch(self.h, None, 0, C.byref(ne))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below
                self._raise(rc, "mfm_runbatch_fetch")
            max_events = ne.value
        evs = np.zeros(max(max_events, 1), RUNBATCH_EVENT_DTYPE)
        rc = self.lib.mfm_runbatch_fetch(self.h, evs.ctypes.data, max_events, C.byref(ne))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runbatch_fetch")
            except MfmError as err:
                err.needed = ne.value
                raise
        return evs[:ne.value].copy()

    def device_view(self):
        """(d_events, d_totals): device addresses of the last call's events and the four uint64 totals (events, runs, overflow,
        input error)"""
        e, t = C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runbatch_device_view(self.h, C.byref(e), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runbatch_device_view")
        return e.value, t.value

    def capacity(self):
        """(max_runs, max_events) fixed at create"""
        r, e = C.c_uint32(), C.c_uint64()
        rc = self.lib.mfm_runbatch_get_capacity(self.h, C.byref(r), C.byref(e))
        if rc < 0:
            self._raise(rc, "mfm_runbatch_get_capacity")
        return r.value, e.value

    def fetch_state(self):
        """the per-channel state the last call left (RUNBATCH_STATE_DTYPE [C]): what the host twin carries"""
        out = np.zeros(self.nr_channels, RUNBATCH_STATE_DTYPE)
        rc = self.lib.mfm_runbatch_fetch_state(self.h, out.ctypes.data, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runbatch_fetch_state")
        return out

    def store_state(self, state, nr_channels=None):
        """mfm_runbatch_store_state: what the next process call continues from.  Validated first: MfmError(MFM_E_INVAL) with a
        message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNBATCH_STATE_DTYPE) if state is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        rc = self.lib.mfm_runbatch_store_state(self.h, st.ctypes.data if st is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runbatch_store_state")


def hosttwin_runbatch_state(nr_channels):
    """the host twin's per-channel state at the start of a stream: RUNBATCH_STATE_DTYPE [C], all zero (no stretch)"""
    return np.zeros(nr_channels, RUNBATCH_STATE_DTYPE)


def hosttwin_runbatch_call(state, runs, bits, sync_events, words, word_mask=0, keep_distance=4, totals=None, max_runs=None,
                           max_decisions=None, max_events=0, max_out_events=None, flags=0, abi_version=MFM_ABI_VERSION):
    """mfm_hosttwin_runbatch_call: one call of the burst batch stage on the CPU.  state (hosttwin_runbatch_state) is updated in
    place; runs RUNSYNC_RUN_DTYPE, bits uint32 and sync_events RUNSYNC_EVENT_DTYPE are one burst sync call's result, totals its four
    totals (default: the lengths, no flags); max_runs / max_decisions / max_events are the configuration's (default: what the call
    needs); returns the RUNBATCH_EVENT_DTYPE events.  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute (overflow
    | input error << 8)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNBATCH_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNSYNC_RUN_DTYPE).reshape(-1)
    bb = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    ee = np.ascontiguousarray(sync_events, dtype=RUNSYNC_EVENT_DTYPE).reshape(-1)
    t = np.array([rr.size, ee.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_decisions = max(int(rr["nr_dec"].astype(np.uint64).sum()), 1) if max_decisions is None else max_decisions
    cfg = _runbatch_config(state.shape[0], max_runs, max_decisions, words, word_mask, keep_distance, max_events, 0, flags, abi_version)
    max_out_events = int((3 * (rr["nr_dec"].astype(np.uint64) // RUNBATCH_FRAME) + 5).sum()) if max_out_events is None else max_out_events
    out_e = np.zeros(max(max_out_events, 1), RUNBATCH_EVENT_DTYPE)
    ne, fl = C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runbatch_call(C.byref(cfg), state.ctypes.data, rr.ctypes.data if rr.size else None, bb.ctypes.data if bb.size else None,
                                        ee.ctypes.data if ee.size else None, t.ctypes.data, out_e.ctypes.data, max_out_events, C.byref(ne),
                                        C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runbatch_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = ne.value, fl.value
        raise err
    return out_e[:ne.value].copy()


def hosttwin_runbatch_state_check(state):
    """mfm_hosttwin_runbatch_state_check: what RunBatch.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNBATCH_STATE_DTYPE).reshape(-1)
    lib = load_library()
    rc = lib.mfm_hosttwin_runbatch_state_check(st.shape[0], st.ctypes.data)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runbatch_state_check", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())


def runbatch_to_pocsag_events(events, baud):
    """mfm_pocsag_event records (POCSAG_EVENT_DTYPE, what host/mfm_pager_pocsag.c's pager_pocsag_on_events takes) from the burst
    batch stage's: `baud` is the caller's (the stage counts decisions, not samples) and sample = dec, stretch-relative: one pager
    object per (channel, stretch), a fresh one at every new stretch_window, as the stage has a fresh automaton there"""
    ev = np.asarray(events)
    assert ev.dtype == RUNBATCH_EVENT_DTYPE
    out = np.zeros(ev.shape, POCSAG_EVENT_DTYPE)
    for f in ("type", "channel", "aux", "nr_ok", "fail_mask", "raw", "corrected"):
        out[f] = ev[f]
    out["baud"] = baud
    out["sample"] = ev["dec"]
    return out


def hosttwin_runpocsag_state(nr_channels):
    """the host twin's per-channel state at the start of a stream: RUNPOCSAG_STATE_DTYPE [C], all zero (no stretch)"""
    return np.zeros(nr_channels, RUNPOCSAG_STATE_DTYPE)


def hosttwin_runpocsag_call(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_out=None):
    """mfm_hosttwin_runpocsag_call: one call of the burst POCSAG stage on the CPU.  state (hosttwin_runpocsag_state) is updated
    in place; runs RUNRS_RUN_DTYPE and payload int16 are one burst resampler call's result, totals its four totals (default:
    the lengths, no flags); max_runs / max_out_samples / max_events are the configuration's (default: what the call needs);
    returns the events.  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute (overflow | input error << 8)"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNPOCSAG_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(payload, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, pl.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(pl.size, 1) if max_out_samples is None else max_out_samples
    if max_out is None:
        max_out = 3 * (pl.size // RUNPOCSAG_MIN_SPACING) + 5 * rr.size
    out = np.zeros(max(max_out, 1), RUNPOCSAG_EVENT_DTYPE)
    nr, fl = C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runpocsag_call(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                         rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                         out.ctypes.data, max_out, C.byref(nr), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runpocsag_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = nr.value, fl.value
        raise err
    return out[:nr.value].copy()


def hosttwin_runpocsag_call_bits(state, runs, bits, polarity=MFM_BITS_NEG, totals=None, max_runs=None, max_out_samples=None, max_events=0,
                                 max_out=None):
    """mfm_hosttwin_runpocsag_call_bits: hosttwin_runpocsag_call on the burst resampler's bits form.  runs (out_offset in words)
    and bits uint32 are one bits call's result, totals its four totals (default: the lengths, no flags); the same state may go
    through PCM and bits calls in turn"""
    lib = load_library()
    state = np.asarray(state)
    assert state.dtype == RUNPOCSAG_STATE_DTYPE and state.flags.c_contiguous and state.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    bw = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    t = np.array([rr.size, bw.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    nout = int(rr["nr_out"].astype(np.uint64).sum())
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(nout, 1) if max_out_samples is None else max_out_samples
    if max_out is None:
        max_out = 3 * (nout // RUNPOCSAG_MIN_SPACING) + 5 * rr.size
    out = np.zeros(max(max_out, 1), RUNPOCSAG_EVENT_DTYPE)
    nr, fl = C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runpocsag_call_bits(state.shape[0], max_runs, max_out_samples, max_events, state.ctypes.data,
                                           rr.ctypes.data if rr.size else None, bw.ctypes.data if bw.size else None, polarity,
                                           t.ctypes.data, out.ctypes.data, max_out, C.byref(nr), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runpocsag_call_bits", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.flags = nr.value, fl.value
        raise err
    return out[:nr.value].copy()


def runpocsag_to_pocsag_events(events):
    """mfm_pocsag_event records (POCSAG_EVENT_DTYPE, what host/mfm_pager_pocsag.c's pager_pocsag_on_events takes) from the burst
    stage's, field for field, the stretch-relative `sample` kept: one pager object per (channel, stretch), a fresh one at
    every new stretch_window, as the stage has a fresh demodulator there"""
    ev = np.asarray(events)
    assert ev.dtype == RUNPOCSAG_EVENT_DTYPE
    out = np.zeros(ev.shape, POCSAG_EVENT_DTYPE)
    for f in ("type", "baud", "channel", "aux", "sample", "nr_ok", "fail_mask", "raw", "corrected"):
        out[f] = ev[f]
    return out


class RunFlex(_RunEnds):
    """mfm_runflex: the runs of a RunResampler's device view (16 000 Hz) through the FLEX front half, one fresh decoder per
    stretch; RUNFLEX_EVENT_DTYPE records and FLEX_FRAME_DTYPE words.  max_runs and max_out_samples are the burst resampler's
    capacities (RunFlex.behind reads them); max_events 0 and max_frames 0 are bounds that cannot overflow."""
    _ends_stage, _ends_dtype = "runflex", RUNFLEX_END_DTYPE

    def __init__(self, nr_channels, max_runs, max_out_samples, max_events=0, max_frames=0, device=0, flags=0,
                 abi_version=MFM_ABI_VERSION):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = RunFlexConfig(abi_version, device, nr_channels, max_runs, max_out_samples, max_events, max_frames, flags)
        rc = self.lib.mfm_runflex_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            self._raise(rc, "mfm_runflex_create")
        self.nr_channels = nr_channels

    @classmethod
    def behind(cls, run_resampler, max_events=0, max_frames=0, device=0):
        """a stage sized for everything one call of `run_resampler` can produce"""
        max_runs, max_out = run_resampler.capacity()
        return cls(run_resampler.nr_channels, max_runs, max_out, max_events=max_events, max_frames=max_frames, device=device)

    def close(self):
        if self.h:
            self.lib.mfm_runflex_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        raise MfmError(rc, what, self.lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else self.lib.mfm_strerror(rc).decode())

    def process_device(self, d_runs, d_payload, d_totals, stream=None):
        """the three addresses of RunResampler.device_view(), after its process_device on the same stream"""
        rc = self.lib.mfm_runflex_process_device(self.h, C.c_void_p(d_runs), C.c_void_p(d_payload), C.c_void_p(d_totals), C.c_void_p(stream or 0))
        if rc < 0:
            self._raise(rc, "mfm_runflex_process_device")

    def fetch(self, max_events=None, max_frames=None):
        """(events, frames) of the last call (RUNFLEX_EVENT_DTYPE, FLEX_FRAME_DTYPE).  With max_events or max_frames too small:
        MfmError(MFM_E_NOMEM) whose `needed` / `needed_frames` attributes are the numbers that would fit and whose `buffer` /
        `frame_buffer` are untouched"""
        ne, nf = C.c_size_t(), C.c_size_t()
        if max_events is None or max_frames is None:
            rc = self.lib.mfm_runflex_fetch(self.h, None, 0, C.byref(ne), None, 0, C.byref(nf))
            if rc not in (MFM_OK, MFM_E_NOMEM, MFM_E_STATE):  # MFM_E_STATE comes again below, with the untouched buffers
                self._raise(rc, "mfm_runflex_fetch")
            max_events = ne.value if max_events is None else max_events
            max_frames = nf.value if max_frames is None else max_frames
        ev = np.zeros(max(max_events, 1), RUNFLEX_EVENT_DTYPE)
        fw = np.zeros(max(max_frames, 1), FLEX_FRAME_DTYPE)
        rc = self.lib.mfm_runflex_fetch(self.h, ev.ctypes.data, max_events, C.byref(ne), fw.ctypes.data, max_frames, C.byref(nf))
        if rc < 0:
            try:
                self._raise(rc, "mfm_runflex_fetch")
            except MfmError as err:
                err.needed, err.needed_frames = ne.value, nf.value
                err.buffer, err.frame_buffer = ev, fw
                raise
        return ev[:ne.value].copy(), fw[:nf.value].copy()

    def device_view(self):
        """(d_events, d_frames, d_totals): device addresses of the last call's events, frame words and the four uint64 totals
        (events, frames, overflow, input error)"""
        e, f, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.mfm_runflex_device_view(self.h, C.byref(e), C.byref(f), C.byref(t))
        if rc < 0:
            self._raise(rc, "mfm_runflex_device_view")
        return e.value, f.value, t.value

    def fetch_state(self, with_ring=True):
        """the per-channel state the last call left (RUNFLEX_STATE_DTYPE [C]) and, with_ring, the rings (int16 [C][32768]): what
        the host twin carries"""
        out = np.zeros(self.nr_channels, RUNFLEX_STATE_DTYPE)
        ring = np.zeros((self.nr_channels, RUNFLEX_RING), np.int16) if with_ring else None
        rc = self.lib.mfm_runflex_fetch_state(self.h, out.ctypes.data, ring.ctypes.data if with_ring else None, self.nr_channels)
        if rc < 0:
            self._raise(rc, "mfm_runflex_fetch_state")
        return (out, ring) if with_ring else out

    def store_state(self, state, ring, nr_channels=None):
        """mfm_runflex_store_state: the state and the rings the next process call continues from.  Validated first:
        MfmError(MFM_E_INVAL) with a message naming channel and field, and nothing written"""
        st = np.ascontiguousarray(state, dtype=RUNFLEX_STATE_DTYPE) if state is not None else None
        rg = np.ascontiguousarray(ring, dtype=np.int16) if ring is not None else None
        n = self.nr_channels if nr_channels is None else nr_channels
        assert st is None or st.shape == (n,)
        assert rg is None or rg.shape == (n, RUNFLEX_RING)
        rc = self.lib.mfm_runflex_store_state(self.h, st.ctypes.data if st is not None else None, rg.ctypes.data if rg is not None else None, n)
        if rc < 0:
            self._raise(rc, "mfm_runflex_store_state")


def hosttwin_runflex_state(nr_channels):
    """the host twin's (state, ring) at the start of a stream: RUNFLEX_STATE_DTYPE [C] and int16 [C][32768], all zero"""
    return np.zeros(nr_channels, RUNFLEX_STATE_DTYPE), np.zeros((nr_channels, RUNFLEX_RING), np.int16)


def hosttwin_runflex_call(state, runs, payload, totals=None, max_runs=None, max_out_samples=None, max_events=0, max_frames=0,
                          max_out=None, max_out_frames=None):
    """mfm_hosttwin_runflex_call: one call of the burst FLEX stage on the CPU.  state = (state, ring) of hosttwin_runflex_state,
    both updated in place; runs RUNRS_RUN_DTYPE and payload int16 are one burst resampler call's result, totals its four totals
    (default: the lengths, no flags); max_runs / max_out_samples / max_events / max_frames are the configuration's (default:
    what the call needs); returns (events, frames).  A refused call raises MfmError(MFM_E_STATE) with a `flags` attribute
    (overflow | input error << 8)"""
    lib = load_library()
    st, ring = state
    assert st.dtype == RUNFLEX_STATE_DTYPE and st.flags.c_contiguous and st.ndim == 1
    assert ring.dtype == np.int16 and ring.flags.c_contiguous and ring.shape == (st.shape[0], RUNFLEX_RING)
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(payload, dtype=np.int16).reshape(-1)
    t = np.array([rr.size, pl.size, 0, 0] if totals is None else totals, np.uint64)
    assert t.shape == (4,)
    max_runs = max(rr.size, 1) if max_runs is None else max_runs
    max_out_samples = max(pl.size, 1) if max_out_samples is None else max_out_samples
    if max_out is None:
        max_out = pl.size // RUNFLEX_EVENT_SPACING + rr.size
    if max_out_frames is None:
        max_out_frames = pl.size // RUNFLEX_FRAME_SPACING + rr.size
    ev = np.zeros(max(max_out, 1), RUNFLEX_EVENT_DTYPE)
    fw = np.zeros(max(max_out_frames, 1), FLEX_FRAME_DTYPE)
    ne, nf, fl = C.c_size_t(), C.c_size_t(), C.c_uint32()
    rc = lib.mfm_hosttwin_runflex_call(st.shape[0], max_runs, max_out_samples, max_events, max_frames, st.ctypes.data, ring.ctypes.data,
                                       rr.ctypes.data if rr.size else None, pl.ctypes.data if pl.size else None, t.ctypes.data,
                                       ev.ctypes.data, max_out, C.byref(ne), fw.ctypes.data, max_out_frames, C.byref(nf), C.byref(fl))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runflex_call", lib.mfm_last_error().decode() if rc in (MFM_E_INVAL, MFM_E_STATE) else lib.mfm_strerror(rc).decode())
        err.needed, err.needed_frames, err.flags = ne.value, nf.value, fl.value
        raise err
    return ev[:ne.value].copy(), fw[:nf.value].copy()


def runflex_to_flex_events(events):
    """mfm_flex_event records (FLEX_EVENT_DTYPE, what host/mfm_pager_flex.c's pager_flex_on_events takes beside the frames) from
    the burst stage's, field for field, the stretch-relative `sample` and `sync_sample` kept: one pager object per (channel,
    stretch), a fresh one at every new stretch_window, as the stage has a fresh decoder there"""
    ev = np.asarray(events)
    assert ev.dtype == RUNFLEX_EVENT_DTYPE
    out = np.zeros(ev.shape, FLEX_EVENT_DTYPE)
    for f in FLEX_EVENT_DTYPE.names:
        out[f] = ev[f]
    return out


def hosttwin_runrs_state(nr_channels, nr_coeffs, interpolate):
    """(state, pending) of the host twin at the start of a stream: RUNRS_STATE_DTYPE [C] and int16 [C][plen]"""
    state = np.zeros(nr_channels, RUNRS_STATE_DTYPE)
    state["expected"] = MFM_RUNRS_NO_WINDOW
    return state, np.zeros((nr_channels, runrs_phase_len(nr_coeffs, interpolate)), np.int16)


def _state_check(what, rc):
    if rc < 0:
        lib = load_library()
        raise MfmError(rc, what, lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())


def hosttwin_runrs_state_check(state, interpolate, plen, dc=None):
    """mfm_hosttwin_runrs_state_check: what RunResampler.store_state validates, on the CPU; MfmError(MFM_E_INVAL) with a message
    naming the first channel and field that fail"""
    st = np.ascontiguousarray(state, dtype=RUNRS_STATE_DTYPE)
    d = np.ascontiguousarray(dc, dtype=RUNRS_DC_STATE_DTYPE) if dc is not None else None
    assert st.ndim == 1 and (d is None or d.shape == st.shape)
    _state_check("mfm_hosttwin_runrs_state_check", load_library().mfm_hosttwin_runrs_state_check(
        st.shape[0], interpolate, plen, st.ctypes.data, d.ctypes.data if d is not None else None))


def hosttwin_runais_state_check(state):
    """mfm_hosttwin_runais_state_check: what RunAis.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNAIS_STATE_DTYPE)
    assert st.ndim == 1
    _state_check("mfm_hosttwin_runais_state_check", load_library().mfm_hosttwin_runais_state_check(st.shape[0], st.ctypes.data))


def hosttwin_runpocsag_state_check(state):
    """mfm_hosttwin_runpocsag_state_check: what RunPocsag.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNPOCSAG_STATE_DTYPE)
    assert st.ndim == 1
    _state_check("mfm_hosttwin_runpocsag_state_check", load_library().mfm_hosttwin_runpocsag_state_check(st.shape[0], st.ctypes.data))


def hosttwin_runflex_state_check(state):
    """mfm_hosttwin_runflex_state_check: what RunFlex.store_state validates, on the CPU"""
    st = np.ascontiguousarray(state, dtype=RUNFLEX_STATE_DTYPE)
    assert st.ndim == 1
    _state_check("mfm_hosttwin_runflex_state_check", load_library().mfm_hosttwin_runflex_state_check(st.shape[0], st.ctypes.data))


def hosttwin_runrs_plan(interpolate, decimate, plen, phase, pending, nr_samples):
    """mfm_hosttwin_runrs_plan: the closed form for arrays of cases; returns (nr_out uint64, phase uint32, pending uint32)"""
    lib = load_library()
    ph = np.ascontiguousarray(phase, dtype=np.uint32)
    pe = np.ascontiguousarray(pending, dtype=np.uint32)
    ns = np.ascontiguousarray(nr_samples, dtype=np.uint64)
    assert ph.shape == pe.shape == ns.shape and ph.ndim == 1
    n = ph.size
    out, pho, peo = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    rc = lib.mfm_hosttwin_runrs_plan(interpolate, decimate, plen, ph.ctypes.data, pe.ctypes.data, ns.ctypes.data, n, out.ctypes.data,
                                     pho.ctypes.data, peo.ctypes.data)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runrs_plan", lib.mfm_strerror(rc).decode())
    return out[:n], pho[:n], peo[:n]


def hosttwin_runrs_call(window_samples, coeffs_q14, interpolate, decimate, state, pending, gate_runs, gate_payload, invert=False,
                        max_runs=None, max_elems=None):
    """mfm_hosttwin_runrs_call: one call of the burst resampler on the CPU.  state RUNRS_STATE_DTYPE [C] and pending int16
    [C][plen] (hosttwin_runrs_state) are updated in place; gate_runs GATE_RUN_DTYPE and gate_payload int16 are one gate call's
    result; returns (runs, payload)"""
    lib = load_library()
    state, pending = np.asarray(state), np.asarray(pending)
    co = np.ascontiguousarray(coeffs_q14, dtype=np.int16)
    assert state.dtype == RUNRS_STATE_DTYPE and state.flags.c_contiguous and pending.dtype == np.int16 and pending.flags.c_contiguous
    nch = state.shape[0]
    assert pending.shape == (nch, runrs_phase_len(max(co.size, 1), max(interpolate, 1)))
    gr = np.ascontiguousarray(gate_runs, dtype=GATE_RUN_DTYPE).reshape(-1)
    gp = np.ascontiguousarray(gate_payload, dtype=np.int16).reshape(-1)
    if max_runs is None:
        max_runs = gr.size
    if max_elems is None:  # a run of n samples that meets p <= plen pending ones produces at most (n + p) I / D + 1 outputs
        max_elems = (gp.size + gr.size * pending.shape[1]) * max(interpolate, 1) // max(decimate, 1) + gr.size
    runs = np.zeros(max(max_runs, 1), RUNRS_RUN_DTYPE)
    payload = np.zeros(max(max_elems, 1), np.int16)
    nr, ne = C.c_size_t(), C.c_size_t()
    rc = lib.mfm_hosttwin_runrs_call(nch, window_samples, interpolate, decimate, int(invert), _i16p(co) if co.size else None, co.size,
                                     state.ctypes.data, _i16p(pending), gr.ctypes.data if gr.size else None, gr.size,
                                     gp.ctypes.data if gp.size else None, gp.size, runs.ctypes.data, max_runs, C.byref(nr),
                                     payload.ctypes.data, max_elems, C.byref(ne))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runrs_call", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())
        err.needed = (nr.value, ne.value)
        raise err
    return runs[:nr.value].copy(), payload[:ne.value].copy()


def hosttwin_runrs_dc_call(pole, dc, runs, payload):
    """mfm_hosttwin_runrs_dc_call: the burst resampler's DC blocker on the CPU, on the (runs, payload) of one
    hosttwin_runrs_call.  dc RUNRS_DC_STATE_DTYPE [C] (zeros at the start of a stream) and payload int16 are updated in
    place; returns payload.  On an error neither is written"""
    lib = load_library()
    dc = np.asarray(dc)
    assert dc.dtype == RUNRS_DC_STATE_DTYPE and dc.flags.c_contiguous and dc.ndim == 1
    rr = np.ascontiguousarray(runs, dtype=RUNRS_RUN_DTYPE).reshape(-1)
    out = np.asarray(payload)
    assert out.dtype == np.int16 and out.flags.c_contiguous and out.ndim == 1
    rc = lib.mfm_hosttwin_runrs_dc_call(dc.shape[0], float(pole), dc.ctypes.data, rr.ctypes.data if rr.size else None, rr.size,
                                        out.ctypes.data if out.size else None, out.size)
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_runrs_dc_call", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())
    return out


def hosttwin_runrs_call_bits(window_samples, coeffs_q14, interpolate, decimate, state, pending, gate_runs, gate_payload, polarity,
                             invert=False, max_runs=None, max_words=None):
    """mfm_hosttwin_runrs_call_bits: hosttwin_runrs_call with the predicate words of `polarity` in the place of the int16:
    returns (runs, bits), out_offset in 32-bit words.  The same state and pending may go through both in turn"""
    lib = load_library()
    state, pending = np.asarray(state), np.asarray(pending)
    co = np.ascontiguousarray(coeffs_q14, dtype=np.int16)
    assert state.dtype == RUNRS_STATE_DTYPE and state.flags.c_contiguous and pending.dtype == np.int16 and pending.flags.c_contiguous
    nch = state.shape[0]
    assert pending.shape == (nch, runrs_phase_len(max(co.size, 1), max(interpolate, 1)))
    gr = np.ascontiguousarray(gate_runs, dtype=GATE_RUN_DTYPE).reshape(-1)
    gp = np.ascontiguousarray(gate_payload, dtype=np.int16).reshape(-1)
    if max_runs is None:
        max_runs = gr.size
    if max_words is None:  # the PCM form's bound on the outputs, / 32, and at most one more word per run
        max_words = ((gp.size + gr.size * pending.shape[1]) * max(interpolate, 1) // max(decimate, 1) + gr.size) // 32 + gr.size
    runs = np.zeros(max(max_runs, 1), RUNRS_RUN_DTYPE)
    bits = np.zeros(max(max_words, 1), np.uint32)
    nr, nw = C.c_size_t(), C.c_size_t()
    rc = lib.mfm_hosttwin_runrs_call_bits(nch, window_samples, interpolate, decimate, int(invert), polarity, _i16p(co) if co.size else None,
                                          co.size, state.ctypes.data, _i16p(pending), gr.ctypes.data if gr.size else None, gr.size,
                                          gp.ctypes.data if gp.size else None, gp.size, runs.ctypes.data, max_runs, C.byref(nr),
                                          bits.ctypes.data, max_words, C.byref(nw))
    if rc < 0:
        err = MfmError(rc, "mfm_hosttwin_runrs_call_bits", lib.mfm_last_error().decode() if rc == MFM_E_INVAL else lib.mfm_strerror(rc).decode())
        err.needed = (nr.value, nw.value)
        raise err
    return runs[:nr.value].copy(), bits[:nw.value].copy()


class Flex:
    """mfm_flex: FLEX sync 1 / FIW / sync 2 / block de-interleave for all channels of a 16 000 Hz PCM block."""

    def __init__(self, nr_channels, max_in_samples, device=0, max_events=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        cfg = FlexConfig(MFM_ABI_VERSION, device, nr_channels, max_in_samples, max_events, 0)
        rc = self.lib.mfm_flex_create(C.byref(self.h), C.byref(cfg))
        if rc < 0:
            raise MfmError(rc, "mfm_flex_create", self.lib.mfm_strerror(rc).decode())
        self.nr_channels = nr_channels
        self.max_events = max_events or (max_in_samples // 1024 + 8)
        self.max_frames = min(self.max_events, max_in_samples // 28672 + 2)

    def close(self):
        if self.h:
            self.lib.mfm_flex_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_host(self, pcm):
        """pcm: int16 [C][n]; returns (events, frames) of this call (FLEX_EVENT_DTYPE, FLEX_FRAME_DTYPE)"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.nr_channels, -1)
        rc = self.lib.mfm_flex_process_host(self.h, _i16p(a), a.shape[1], a.shape[1])
        if rc < 0:
            raise MfmError(rc, "mfm_flex_process_host", self.lib.mfm_strerror(rc).decode())
        return self.fetch_events()

    def process_device(self, d_pcm, in_stride, nr_in, stream=None):
        rc = self.lib.mfm_flex_process_device(self.h, C.c_void_p(d_pcm), in_stride, nr_in, C.c_void_p(stream or 0))
        if rc < 0:
            raise MfmError(rc, "mfm_flex_process_device", self.lib.mfm_strerror(rc).decode())

    def seek(self, samples_before):
        """mfm_flex_seek: a fresh stage whose next sample has index samples_before (added to sample and sync_sample)"""
        rc = self.lib.mfm_flex_seek(self.h, int(samples_before))
        if rc < 0:
            raise MfmError(rc, "mfm_flex_seek", self.lib.mfm_last_error().decode() or self.lib.mfm_strerror(rc).decode())

    def fetch_events(self):
        cap_e, cap_f = self.nr_channels * self.max_events, self.nr_channels * self.max_frames
        ev = np.zeros(cap_e, FLEX_EVENT_DTYPE)
        fw = np.zeros(cap_f, FLEX_FRAME_DTYPE)
        ne, nf = C.c_size_t(), C.c_size_t()
        rc = self.lib.mfm_flex_fetch_events(self.h, ev.ctypes.data, cap_e, C.byref(ne), fw.ctypes.data, cap_f, C.byref(nf))
        if rc < 0:
            raise MfmError(rc, "mfm_flex_fetch_events", self.lib.mfm_strerror(rc).decode())
        return ev[:ne.value].copy(), fw[:nf.value].copy()


def bch3121_decode(words, device=0):
    """bch_code_decode on the GPU: returns (corrected uint32 array, rc uint8 array)"""
    lib = load_library()
    w = np.ascontiguousarray(words, dtype=np.uint32).copy()
    rc = np.zeros(w.size, np.uint8)
    r = lib.mfm_bch3121_decode_host(w.ctypes.data_as(C.POINTER(C.c_uint32)), rc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    w.size, device)
    if r < 0:
        raise MfmError(r, "mfm_bch3121_decode_host", lib.mfm_strerror(r).decode())
    return w, rc


def hosttwin_splice_bits(window, off0, src, nr_bits):
    """mfm_hosttwin_splice_bits on a copy of `window` (uint32 words): bits [off0, off0 + nr_bits) from `src`"""
    lib = load_library()
    w = np.ascontiguousarray(window, dtype=np.uint32).copy()
    sw = np.ascontiguousarray(src, dtype=np.uint32)
    if sw.size == 0:
        sw = np.zeros(1, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    lib.mfm_hosttwin_splice_bits(w.ctypes.data_as(u32p), int(off0), sw.ctypes.data_as(u32p), int(nr_bits))
    return w


def _resampler_config(coeffs_q14, interpolate, decimate, max_in_samples, nr_channels, invert, dc_pole, force_dot2):
    cfg = ResamplerConfig(MFM_ABI_VERSION, 0, nr_channels, interpolate, decimate, max_in_samples, int(invert),
                          int(dc_pole is not None), float(dc_pole or 0.0), MFM_RS_FORCE_DOT2 if force_dot2 else 0, 0)
    return cfg, np.ascontiguousarray(coeffs_q14, dtype=np.int16)


def hosttwin_resampler_form(coeffs_q14, interpolate, decimate, max_in_samples, nr_channels=1, invert=False, dc_pole=None,
                            force_dot2=False):
    """mfm_hosttwin_resampler_form as a dict: the form Resampler(...) would run, planned without a device; MfmError(MFM_E_INVAL)
    for what create refuses"""
    lib = load_library()
    cfg, co = _resampler_config(coeffs_q14, interpolate, decimate, max_in_samples, nr_channels, invert, dc_pole, force_dot2)
    f = ResamplerForm()
    rc = lib.mfm_hosttwin_resampler_form(C.byref(cfg), _i16p(co), co.size, C.byref(f))
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_resampler_form", lib.mfm_last_error().decode() or lib.mfm_strerror(rc).decode())
    return f.as_dict()


def hosttwin_resampler_matrix_block(coeffs_q14, interpolate, decimate, phase, x):
    """mfm_hosttwin_resampler_matrix_block: the 16 outputs of one block of the matrix form at carried phase `phase`, from the
    tables its kernel reads; x int16, x[0] the block's first sample"""
    lib = load_library()
    cfg, co = _resampler_config(coeffs_q14, interpolate, decimate, 1024, 1, False, None, False)
    xs = np.ascontiguousarray(x, dtype=np.int16)
    y = np.zeros(16, np.int16)
    rc = lib.mfm_hosttwin_resampler_matrix_block(C.byref(cfg), _i16p(co), co.size, int(phase), _i16p(xs), xs.size, _i16p(y))
    if rc < 0:
        raise MfmError(rc, "mfm_hosttwin_resampler_matrix_block", lib.mfm_strerror(rc).decode())
    return y


def hosttwin_bch3121_decode(word):
    lib = load_library()
    v = C.c_uint32(int(word))
    rc = lib.mfm_hosttwin_bch3121_decode(C.byref(v))
    return rc, v.value
