"""liodom_amd — MI355X-native LiODOM hot path (edge extraction, edge-to-line correspondence,
pose solve, sliding-window map) behind the C-ABI of include/liodom_hip.h.

This package is a thin ctypes binding of liodom_amd/lib/libliodom_hip.so (hand-written HIP
kernels for gfx950, liodom_amd/csrc/).  There is no CPU fallback: importing works anywhere, but
`load()` raises if the library has not been built and `Liodom(...)` raises without a GPU.
"""
from . import api  # noqa: F401
from .api import (Places, PlaceGeometry, PlaceMatch, PlacePolicy, PLACE_MATCH_DTYPE, Config, MapHit, MAP_HIT_DTYPE, TrackPolicy, TRACKING, LOST, HIT_VALID, HIT_NO_READER, HIT_NO_SOLVE, device_count, device_pci_bus_id, KernelStat, Liodom, Map, MapConfig, MapperOptions, make_mapper_options, LiodomError, LmTrace, Params, PoseCov, StepInfo, build, lib_path,  # noqa: F401
                  load, make_config, make_params, parse_stream_state, parse_map_state, build_map_state, join_map_state, PolarGeometry, PolarLayout, polar_geometry,
                  polar_geometry_from_angles, polar_layout, pack_polar,
                  RegisterOptions, Registration, make_register_options, registration_dict,
                  PoseGraph, GraphEdge, GraphOptions, GraphReport, GRAPH_EDGE_DTYPE, GRAPH_TERMINATIONS, graph_edges, make_graph_options,
                  GraphCovOptions, GRAPH_COV_STATUSES, GRAPH_COV_STATUS_DTYPE, make_graph_cov_options)
