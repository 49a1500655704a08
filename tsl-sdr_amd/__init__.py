"""MI355X-native multifm channel engine (drop-in for pvachon/tsl-sdr's multifm hot path).

The product is libmultifm_hip.so (csrc/, behind include/multifm_hip.h) and the C host in host/.
This Python package only carries the ctypes mirror of that C ABI and the synthetic-input helpers
that tests/ and bench.py share.  The directory name has a hyphen, so load it with
`__graft_entry__.load_package()` (importlib), which registers it as `tsl_sdr_amd`.
"""
from . import binding, dist, synth  # noqa: F401
from .binding import Ais, BitsView, Engine, F32Engine, Flex, Gate, GateConfig, GATE_RUN_DTYPE, MFM_GATE_MAX_PREROLL, Group, Level, LevelConfig, LEVEL_RECORD_DTYPE, MfmError, MuellerMuller, Pocsag, Resampler, RunAis, RunFlex, RunFlexConfig, RunPocsag, RunPocsagConfig, RunResampler, RunRouter, MFM_ROUTE_NONE, MFM_RUNROUTE_MAX_ROUTES, RUNAIS_EVENT_DTYPE, RUNFLEX_EVENT_DTYPE, RUNFLEX_STATE_DTYPE, RUNPOCSAG_EVENT_DTYPE, RUNPOCSAG_STATE_DTYPE, RUNRS_DC_STATE_DTYPE, RUNRS_RUN_DTYPE, hosttwin_runais_call, hosttwin_runflex_call, hosttwin_runflex_state, hosttwin_runpocsag_call, hosttwin_runpocsag_state, hosttwin_runrs_call, hosttwin_runais_call_bits, hosttwin_runpocsag_call_bits, hosttwin_runrs_call_bits, hosttwin_runrs_dc_call, hosttwin_runroute_call, hosttwin_runroute_capacity, hosttwin_runroute_route_caps, hosttwin_runroute_sets_call, hosttwin_runroute_local_call, MFM_RUNROUTE_F_PACK, RunrsBitsView, load_library, runflex_event_bound, runflex_frame_bound, runflex_to_flex_events, runpocsag_to_pocsag_events, RUNAIS_END_DTYPE, RUNPOCSAG_END_DTYPE, RUNFLEX_END_DTYPE, hosttwin_runais_call_ends, hosttwin_runpocsag_call_ends, hosttwin_runflex_call_ends, hosttwin_runais_end_stretches, hosttwin_runpocsag_end_stretches, hosttwin_runflex_end_stretches  # noqa: F401
