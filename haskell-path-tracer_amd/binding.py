"""ctypes binding of include/ptmi.h -- the Python face of the C ABI used by tests and bench.py.

This is a thin mirror: one method per entry point, numpy arrays for host planes, optional
torch tensors for caller-owned device planes (torch is plumbing for device memory, streams and
torch.distributed only).  There is no fallback: if libptmi.so is missing or no GPU is present
the calls raise PtmiError.
"""
import ctypes as C
import os

import numpy as np

from . import _build
from .world import CAMERA_DTYPE, PLANE_DTYPE, SPHERE_DTYPE, TRIANGLE_DTYPE, INLINE, STREAMS, triangle  # noqa: F401

OPT_STREAMS_SEED_RULE, OPT_STREAM_STEP_CAP, OPT_STREAM_CAPACITY, OPT_STREAMS_FORM, OPT_STREAM_BATCH, OPT_SPP_CHUNKS, OPT_ARITHMETIC = 1, 2, 3, 4, 5, 6, 7
OPT_STREAM_TAIL, OPT_ORDERED_PASSES, OPT_GLASS_BATCH, OPT_STREAM_GRADED, OPT_SNAPSHOT_BUDGET_MB, OPT_STREAM_PASS_GROUPS, OPT_CHAIN_SLOTS, OPT_PASS_HANDOFF = 8, 9, 10, 11, 12, 13, 14, 15
OPT_BVH_DEVICE_BUILD = 17                                        # (16 is unused)
BVH_BUILD_EQUAL_COUNT, BVH_BUILD_SPATIAL = 0, 1
CHAIN_CONSUME = 1
HANDOFF_FENCED, HANDOFF_FENCE_FREE = 0, 1
ARITH_EXACT, ARITH_CONTRACTED = 0, 1
SEED_KEEP_ACCUMULATOR, SEED_FROM_RESULT, SEED_AUTO = 0, 1, 2
FORM_AUTO, FORM_STREAM, FORM_PIXEL = 0, 1, 2
PTMI_OK, PTMI_EINVAL, PTMI_ENODEVICE, PTMI_EHIP, PTMI_ENOMEM, PTMI_ESTATE, PTMI_ELIMIT, PTMI_ESTALE = 0, -1, -2, -3, -4, -5, -6, -7
MAX_PRIMITIVES, MAX_BVH_SPHERES, MAX_BVH_PLANES, BVH_MAX_DEPTH, BVH_LEAF_MAX = 1024, 1 << 22, 64, 24, 4
MAX_MESH_TRIANGLES = 1 << 22
RAY_ORDER_MAX = 1 << 22
MULTI_HIT_MAX = 16                                               # PTMI_MULTI_HIT_MAX: the longest list ptmi_trace_rays_multi_device keeps per ray
RAY_KEY_NOT_PLACED = 1 << 44                                     # ptmi_ray_order_keys: a ray with a non-finite word or a zero direction
# ptmi_bvh_node: the boxes of both children (centre, half extent), the child references, 1 / (2 r_min) per child
BVH_NODE_DTYPE = np.dtype([("center", "<f4", (2, 3)), ("half", "<f4", (2, 3)), ("ref", "<i4", 2), ("inv_2r", "<f4", 2)])

# every symbol include/ptmi.h declares: name -> (restype, argtypes)
_f32p, _u32p, _i32p, _i64p, _vp = (C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64), C.c_void_p)


class Stats(C.Structure):
    _fields_ = [("live_bounces", C.c_uint64), ("nominal_bounces", C.c_uint64), ("samples", C.c_uint64),
                ("last_render_ms", C.c_float), ("stream_iterations", C.c_uint32), ("stream_rays_dropped", C.c_uint64),
                ("stream_rays_truncated", C.c_uint64), ("stream_rays_spilled", C.c_uint64), ("stream_rays_overflowed", C.c_uint64)]


class ChainStats(C.Structure):
    _fields_ = [("states_on_device", C.c_uint32), ("states_on_host", C.c_uint32), ("device_slots", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("renders_chained", C.c_uint64), ("renders_in_place", C.c_uint64), ("renders_uploaded", C.c_uint64), ("evictions", C.c_uint64), ("fetches", C.c_uint64)]


SYMBOLS = {
    "ptmi_version": (C.c_int, []),
    "ptmi_build_id": (C.c_char_p, []),
    "ptmi_strerror": (C.c_char_p, [C.c_int]),
    "ptmi_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "ptmi_destroy": (None, [_vp]),
    "ptmi_last_error": (C.c_char_p, [_vp]),
    "ptmi_set_scene": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_set_scene_bvh": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_bvh_layout": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp]),
    "ptmi_set_scene_mesh": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_mesh_layout": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    "ptmi_update_mesh_vertices": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_update_mesh_vertices_device": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_mesh_refit_layout": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_mesh_read_layout": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "ptmi_set_mesh_triangles": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_set_mesh_triangles_device": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_mesh_layout_morton": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    "ptmi_update_spheres": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_update_spheres_device": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_set_bvh_spheres": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_set_bvh_spheres_device": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_bvh_refit_layout": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp]),
    "ptmi_bvh_layout_morton": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp]),
    "ptmi_bvh_layout_spatial": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp]),
    "ptmi_bvh_read_layout": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "ptmi_resize": (C.c_int, [_vp, C.c_int, C.c_int]),
    "ptmi_set_partition": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "ptmi_local_rows": (C.c_int, [_vp]),
    "ptmi_global_row": (C.c_int, [_vp, C.c_int]),
    "ptmi_bind_planes": (C.c_int, [_vp] + [_vp] * 7),
    "ptmi_get_planes": (C.c_int, [_vp] + [C.POINTER(_vp)] * 7),
    "ptmi_set_stream": (C.c_int, [_vp, _vp]),
    "ptmi_set_timing": (C.c_int, [_vp, C.c_int]),
    "ptmi_set_variant": (C.c_int, [_vp, C.c_int]),
    "ptmi_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "ptmi_get_option": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    "ptmi_init_output": (C.c_int, [_vp, C.c_uint64]),
    "ptmi_reseed": (C.c_int, [_vp, C.c_uint64]),
    "ptmi_create_with": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ptmi_upload_state": (C.c_int, [_vp] + [_vp] * 7),
    "ptmi_download_state": (C.c_int, [_vp] + [_vp] * 7),
    "ptmi_download_color": (C.c_int, [_vp] + [_vp] * 3),
    "ptmi_render": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    "ptmi_synchronize": (C.c_int, [_vp]),
    "ptmi_render_blocks": (C.c_int, [_vp, C.c_int]),
    "ptmi_render1": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp] + [_vp] * 14),
    "ptmi_render1_chained": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int] + [_vp] * 7 + [C.POINTER(C.c_uint64)] + [_vp] * 7),
    "ptmi_chain_init_output": (C.c_int, [_vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ptmi_chain_reseed": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "ptmi_chain_fetch": (C.c_int, [_vp, C.c_uint64] + [_vp] * 7),
    "ptmi_chain_release": (C.c_int, [_vp, C.c_uint64]),
    "ptmi_chain_info": (C.c_int, [_vp, C.POINTER(ChainStats)]),
    "ptmi_present": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "ptmi_snapshot_color": (C.c_int, [_vp, _vp, _vp]),
    "ptmi_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "ptmi_group_create": (C.c_int, [C.POINTER(_vp), _i32p, C.c_int, C.c_int]),
    "ptmi_group_destroy": (None, [_vp]),
    "ptmi_group_size": (C.c_int, [_vp]),
    "ptmi_group_member": (_vp, [_vp, C.c_int]),
    "ptmi_group_last_error": (C.c_char_p, [_vp]),
    "ptmi_group_set_scene": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_group_set_scene_bvh": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_group_set_scene_mesh": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int]),
    "ptmi_group_update_mesh_vertices": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_group_set_mesh_triangles": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_group_update_spheres": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_group_set_bvh_spheres": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_group_resize": (C.c_int, [_vp, C.c_int, C.c_int]),
    "ptmi_group_init_output": (C.c_int, [_vp, C.c_uint64]),
    "ptmi_group_reseed": (C.c_int, [_vp, C.c_uint64]),
    "ptmi_group_render": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    "ptmi_group_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "ptmi_group_set_variant": (C.c_int, [_vp, C.c_int]),
    "ptmi_group_synchronize": (C.c_int, [_vp]),
    "ptmi_group_download_color": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ptmi_group_gather_color": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_group_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "ptmi_partition_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ptmi_partition_global_row": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ptmi_reset_stats": (C.c_int, [_vp]),
    "ptmi_debug_counters": (C.c_int, [_vp, _vp]),
    "ptmi_debug_counters_n": (C.c_int, [_vp, _vp, C.c_int]),
    "ptmi_order_schedule": (C.c_int, [C.c_int, C.c_int, _i32p, _i32p]),
    "ptmi_stream_schedule": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _vp, C.c_int]),
    "ptmi_stream_tickets": (C.c_int, [C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int]),
    "ptmi_eval_distance_to_sphere": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_eval_distance_to_plane": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_eval_check_hit": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_trace_rays_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_occluded_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "ptmi_ray_order_bytes": (C.c_size_t, [C.c_int]),
    "ptmi_ray_order_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_size_t]),
    "ptmi_ray_order": (C.c_int, [_vp, C.c_int, _vp]),
    "ptmi_ray_order_keys": (C.c_int, [_vp, C.c_int, _vp]),
    "ptmi_trace_rays_indexed_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_occluded_indexed_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp]),
    "ptmi_trace_rays_multi_device": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "ptmi_trace_rays_multi_indexed_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "ptmi_nearest_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_nearest_indexed_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_nearest": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "ptmi_path_seeds_device": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "ptmi_trace_paths_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "ptmi_trace_paths_indexed_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "ptmi_bounce_rays_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ptmi_bounce_rays_indexed_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ptmi_live_rays_bytes": (C.c_size_t, [C.c_int]),
    "ptmi_live_rays_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_size_t]),
    "ptmi_live_rays": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    "ptmi_trace_streams_bytes": (C.c_size_t, [C.c_int]),
    "ptmi_trace_streams_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    "ptmi_trace_streams_indexed_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    "ptmi_eval_sincos": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "ptmi_eval_quaternion": (C.c_int, [_vp, _vp, C.c_int, _vp]),
}


class PtmiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libptmi error %d: %s" % (code, message))
        self.code = code


_lib = None


def open_library(path, check_build_id=True):
    """dlopen one libptmi build and type every symbol (a second build -- the ablation library, a diagnostic build -- can be
    open beside the default one: Context(library=...)).
    The library must hold the code the sources beside this file compile to: either it was linked from this very text, or its
    ptmi_build_id() -- a hash over the compiled objects' code (_build.code_id) -- is what the sources give now (a comment edit
    keeps it).  A binary that travelled with edited kernels, or one from an older checkout, is refused here instead of being
    measured under the wrong name."""
    if not os.path.exists(path):
        raise PtmiError(PTMI_ESTATE, "libptmi.so not built (%s); run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    lib.build_id = (lib.ptmi_build_id() or b"").decode("ascii", "replace")
    if check_build_id and not _build.matches_sources(path):
        raise PtmiError(PTMI_ESTATE, "%s was built from other sources: it carries build id %r (linked from text %r), the sources here "
                                     "have text hash %r and do not compile to that code; rebuild it (__graft_entry__.build())"
                        % (path, lib.build_id, _build.read_source_hash(path), _build.source_hash()))
    return lib


def load_library(path=None, check_build_id=True):
    """The default library of the process: libptmi.so (building nothing: see _build.build_lib), or `path` from then on.
    check_build_id=False only for tools that compare binaries of DIFFERENT sources on purpose (tools/ab.py prints each one's id)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    _lib = open_library(path or _build.LIB, check_build_id)
    return _lib


def stream_schedule(n_spp, n_pixels, lanes, batch=0, graded=True):
    """ptmi_stream_schedule: the first sample of every pass of the stream form's split kernel, and n_spp behind them (host arithmetic)."""
    first = np.zeros(65, np.int32)
    passes = load_library().ptmi_stream_schedule(int(n_spp), int(n_pixels), int(lanes), int(batch), 1 if graded else 0, _ptr(first), 65)
    if passes < 0:
        raise PtmiError(passes, "ptmi_stream_schedule")
    return [int(v) for v in first[:passes + 1]]


def stream_tickets(option, first, queue_regions):
    """ptmi_stream_tickets: [(pass, region index within the queue)] in the order one ticket queue of the split kernel hands them out, for
    the schedule `first` of stream_schedule."""
    passes = len(first) - 1
    n = passes * queue_regions
    f = np.asarray(first, np.int32)
    p, r = np.zeros(n, np.int32), np.zeros(n, np.int32)
    got = load_library().ptmi_stream_tickets(int(option), _ptr(f), passes, int(queue_regions), _ptr(p), _ptr(r), n)
    if got < 0:
        raise PtmiError(got, "ptmi_stream_tickets")
    return list(zip(p[:got].tolist(), r[:got].tolist()))


def bvh_layout(spheres):
    """ptmi_bvh_layout: the hierarchy ptmi_set_scene_bvh builds over these spheres (host code, no device) -> (nodes as a
    BVH_NODE_DTYPE array, node 0 the root; order: the original index of every position of the leaf order)."""
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    nodes = np.zeros(max(1, s.size), BVH_NODE_DTYPE)
    order = np.zeros(s.size, np.int32)
    got = load_library().ptmi_bvh_layout(_ptr(s) if s.size else None, s.size, _ptr(nodes), nodes.size, _ptr(order) if s.size else None)
    if got < 0:
        raise PtmiError(got, "ptmi_bvh_layout")
    return nodes[:got].copy(), order


def bvh_layout_morton(spheres):
    """ptmi_bvh_layout_morton: the hierarchy ptmi_set_bvh_spheres builds on the device (host code, no device) -> (nodes, order) as
    bvh_layout returns them."""
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    nodes = np.zeros(max(1, s.size), BVH_NODE_DTYPE)
    order = np.zeros(s.size, np.int32)
    got = load_library().ptmi_bvh_layout_morton(_ptr(s) if s.size else None, s.size, _ptr(nodes), nodes.size, _ptr(order) if s.size else None)
    if got < 0:
        raise PtmiError(got, "ptmi_bvh_layout_morton")
    return nodes[:got].copy(), order


def bvh_layout_spatial(spheres):
    """ptmi_bvh_layout_spatial: the hierarchy ptmi_set_bvh_spheres builds on the device under OPT_BVH_DEVICE_BUILD = BVH_BUILD_SPATIAL (host
    code, no device) -> (nodes, order) as bvh_layout returns them."""
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    nodes = np.zeros(max(1, s.size), BVH_NODE_DTYPE)
    order = np.zeros(s.size, np.int32)
    got = load_library().ptmi_bvh_layout_spatial(_ptr(s) if s.size else None, s.size, _ptr(nodes), nodes.size, _ptr(order) if s.size else None)
    if got < 0:
        raise PtmiError(got, "ptmi_bvh_layout_spatial")
    return nodes[:got].copy(), order


def bvh_refit_layout(spheres, nodes, order):
    """ptmi_bvh_refit_layout: `nodes` and `order` of bvh_layout (or bvh_layout_morton) for the scene as set, refitted to the moved
    `spheres` (host code, no device) -> the nodes with new boxes and inv_2r (a copy; ref and order are kept)."""
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    out = np.array(nodes, dtype=BVH_NODE_DTYPE, copy=True).reshape(-1)
    o = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
    rc = load_library().ptmi_bvh_refit_layout(_ptr(s) if s.size else None, s.size, _ptr(out), out.size, _ptr(o) if o.size else None)
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_bvh_refit_layout")
    return out


def _host_rays(rays):
    """(n, 6) float32 host rays -> a contiguous array"""
    r = np.asarray(rays)
    if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != 6 or not r.flags.c_contiguous:
        raise ValueError("rays must be a contiguous float32 array of shape (n, 6), not %s %r" % (r.dtype, r.shape))
    return r


def ray_order_keys(rays):
    """ptmi_ray_order_keys: the key every ray of the batch is ordered by (host code, no device; csrc/ptmi_ray_order.h states it) -> uint64
    (n,), RAY_KEY_NOT_PLACED for a ray with a non-finite word or a zero direction."""
    r = _host_rays(rays)
    keys = np.zeros(r.shape[0], np.uint64)
    rc = load_library().ptmi_ray_order_keys(_ptr(r) if r.size else None, r.shape[0], _ptr(keys) if r.size else None)
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_ray_order_keys")
    return keys


def ray_order(rays):
    """ptmi_ray_order: the order ptmi_ray_order_device gives the batch (host code, no device) -> int32 (n,): the ray of every position,
    ascending by (key, index)."""
    r = _host_rays(rays)
    order = np.zeros(r.shape[0], np.int32)
    rc = load_library().ptmi_ray_order(_ptr(r) if r.size else None, r.shape[0], _ptr(order) if r.size else None)
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_ray_order")
    return order


def ray_order_bytes(n):
    """ptmi_ray_order_bytes: the workspace ptmi_ray_order_device needs for n rays."""
    return int(load_library().ptmi_ray_order_bytes(int(n)))


LIVE_RAYS_MAX = 1 << 22                                    # PTMI_LIVE_RAYS_MAX


def live_rays_bytes(count):
    """ptmi_live_rays_bytes: the workspace ptmi_live_rays_device needs for that many candidates."""
    return int(load_library().ptmi_live_rays_bytes(int(count)))


def live_rays(throughput, index=None, out=None):
    """ptmi_live_rays: the list ptmi_live_rays_device gives (host code, no device) -> (live, count).  throughput: float32 (n, 3); index:
    int32 (m,) or None for the candidates 0 .. n - 1.  live: int32, one entry per candidate -- those inside [0, n) whose throughput is
    not nearZero, in candidate order, then -1 -- written into `out` when given (which may be `index` itself)."""
    t = np.asarray(throughput)
    if t.dtype != np.float32 or t.ndim != 2 or t.shape[1] != 3 or not t.flags.c_contiguous:
        raise ValueError("throughput must be a contiguous float32 array of shape (n, 3), not %s %r" % (t.dtype, t.shape))
    if index is not None:
        index = np.asarray(index)
        if index.dtype != np.int32 or index.ndim != 1 or not index.flags.c_contiguous:
            raise ValueError("index must be a contiguous int32 array of shape (m,), not %s %r" % (index.dtype, index.shape))
    candidates = t.shape[0] if index is None else index.shape[0]
    if out is None:
        out = np.zeros(candidates, np.int32)
    if not isinstance(out, np.ndarray) or out.dtype != np.int32 or out.shape != (candidates,) or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous int32 array of shape (%d,)" % candidates)
    if candidates == 0:                                  # (an empty index has no pointer, and a NULL index means every ray)
        return out, 0
    count = C.c_int32(0)
    rc = load_library().ptmi_live_rays(_ptr(t) if t.size else None, t.shape[0], _ptr(index) if index is not None and index.size else None,
                                       index.shape[0] if index is not None else 0, _ptr(out) if out.size else None, C.byref(count))
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_live_rays")
    return out, int(count.value)


def nearest(spheres, planes, triangles, points, r_max=None, point=False):
    """ptmi_nearest: the nearest-primitive query's host twin (host code, no device) -- for every point the primitive with the least
    (|signed distance|, index) within its r_max, by enumeration.  spheres, planes, triangles: arrays of the scene dtypes (any may be empty
    or None, not all); points: float32 (n, 3); r_max: float32 (n,) or None for no limit.
    -> (dist, idx), or (dist, idx, point) with point=True: dist float32 (n,) the signed distance, negative behind the surface; idx int32
    (n,) -- spheres, then planes, then triangles; a miss is dist 0, idx -1, location (0, 0, 0) -- and point float32 (n, 3), the nearest
    location on the primitive."""
    s = np.ascontiguousarray(spheres if spheres is not None else [], dtype=SPHERE_DTYPE).reshape(-1)
    pl = np.ascontiguousarray(planes if planes is not None else [], dtype=PLANE_DTYPE).reshape(-1)
    t = np.ascontiguousarray(triangles if triangles is not None else [], dtype=TRIANGLE_DTYPE).reshape(-1)
    pts = np.asarray(points)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] != 3 or not pts.flags.c_contiguous:
        raise ValueError("points must be a contiguous float32 array of shape (n, 3), not %s %r" % (pts.dtype, pts.shape))
    n = pts.shape[0]
    if r_max is not None:
        r_max = np.asarray(r_max)
        if r_max.dtype != np.float32 or r_max.shape != (n,) or not r_max.flags.c_contiguous:
            raise ValueError("r_max must be a contiguous float32 array of shape (%d,), not %s %r" % (n, r_max.dtype, r_max.shape))
    dist, idx = np.zeros(n, np.float32), np.zeros(n, np.int32)
    at = np.zeros((n, 3), np.float32) if point else None
    rc = load_library().ptmi_nearest(_ptr(s) if s.size else None, s.size, _ptr(pl) if pl.size else None, pl.size, _ptr(t) if t.size else None, t.size,
                                     _ptr(pts) if n else None, _ptr(r_max) if r_max is not None and n else None, n, _ptr(dist) if n else None,
                                     _ptr(idx) if n else None, _ptr(at) if point and n else None)
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_nearest")
    return (dist, idx, at) if point else (dist, idx)


def _device_rows(t, words, what):
    """a contiguous float32 device tensor of n * words elements (anything with is_cuda and data_ptr()) -> (pointer, n)"""
    if not t.is_cuda or not t.is_contiguous() or "float32" not in str(t.dtype) or t.numel() % words:
        raise ValueError("device %s must be a contiguous float32 tensor of shape (n, %d) on the context's device" % (what, words))
    return _vp(t.data_ptr()), t.numel() // words


def _device_tensor(t, dtype, shape, what):
    """a contiguous device tensor of this dtype ("float32", "int32") and shape, None standing for any length (anything with is_cuda,
    is_contiguous(), dtype, shape, numel() and data_ptr()) -> its pointer, None for an empty one"""
    ok = (hasattr(t, "is_cuda") and hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() and str(t.dtype).split(".")[-1] == dtype
          and len(t.shape) == len(shape) and all(want is None or int(got) == want for got, want in zip(t.shape, shape)))
    if not ok:
        raise ValueError("%s must be a contiguous %s device tensor of shape (%s) on the context's device"
                         % (what, dtype, ", ".join("n" if w is None else str(w) for w in shape)))
    return _vp(t.data_ptr()) if t.numel() else None


def mesh_layout(triangles):
    """ptmi_mesh_layout: the triangle hierarchy ptmi_set_scene_mesh builds (host code, no device) -> (nodes as a BVH_NODE_DTYPE array,
    node 0 the root; order: the original index of every position of the leaf order -- triangles of zero area are in no leaf)."""
    t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    nodes = np.zeros(max(1, t.size), BVH_NODE_DTYPE)
    order = np.zeros(max(1, t.size), np.int32)
    kept = C.c_int(0)
    got = load_library().ptmi_mesh_layout(_ptr(t) if t.size else None, t.size, _ptr(nodes), nodes.size, _ptr(order) if t.size else None,
                                          C.byref(kept))
    if got < 0:
        raise PtmiError(got, "ptmi_mesh_layout")
    return nodes[:got].copy(), order[:kept.value].copy()


def mesh_layout_morton(triangles):
    """ptmi_mesh_layout_morton: the triangle hierarchy ptmi_set_mesh_triangles builds on the device (host code, no device) -> (nodes, order)
    as mesh_layout returns them."""
    t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    nodes = np.zeros(max(1, t.size), BVH_NODE_DTYPE)
    order = np.zeros(max(1, t.size), np.int32)
    kept = C.c_int(0)
    got = load_library().ptmi_mesh_layout_morton(_ptr(t) if t.size else None, t.size, _ptr(nodes), nodes.size, _ptr(order) if t.size else None,
                                                 C.byref(kept))
    if got < 0:
        raise PtmiError(got, "ptmi_mesh_layout_morton")
    return nodes[:got].copy(), order[:kept.value].copy()


def mesh_refit_layout(triangles, nodes, order):
    """ptmi_mesh_refit_layout: `nodes` and `order` of mesh_layout for the scene as set, refitted to the moved `triangles` (host code, no
    device) -> the nodes with new boxes (a copy; ref and order are kept)."""
    t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    out = np.array(nodes, dtype=BVH_NODE_DTYPE, copy=True).reshape(-1)
    o = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
    rc = load_library().ptmi_mesh_refit_layout(_ptr(t) if t.size else None, t.size, _ptr(out), out.size, _ptr(o) if o.size else None, o.size)
    if rc != PTMI_OK:
        raise PtmiError(rc, "ptmi_mesh_refit_layout")
    return out


def _vertex_array(v):
    """(n, 3, 3) or (n, 9) float32 vertices, v0 v1 v2 per triangle -> a contiguous array and n"""
    a = np.ascontiguousarray(v, dtype=np.float32)
    if a.ndim < 2 or a.size != a.shape[0] * 9:
        raise ValueError("vertices must have shape (n, 3, 3) or (n, 9), not %r" % (a.shape,))
    return a, a.shape[0]


def _device_vertices(v):
    """a contiguous float32 device tensor of n * 9 elements (anything with is_cuda and data_ptr()) -> (pointer, n)"""
    if not v.is_cuda or not v.is_contiguous() or "float32" not in str(v.dtype) or v.numel() % 9:
        raise ValueError("device vertices must be a contiguous float32 tensor of shape (n, 3, 3) or (n, 9) on the context's device")
    return _vp(v.data_ptr()), v.numel() // 9


def _device_triangles(t):
    """a contiguous float32 device tensor of shape [n, 15], brdf_tag as its int32 bit pattern (anything with is_cuda and data_ptr()) ->
    (pointer, n)"""
    if not t.is_cuda or not t.is_contiguous() or "float32" not in str(t.dtype) or t.numel() % 15:
        raise ValueError("device triangles must be a contiguous float32 tensor of shape (n, 15) on the context's device")
    return _vp(t.data_ptr()), t.numel() // 15


def _mesh_args(spheres, triangles, planes):
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE).reshape(-1)
    return (s, t, p), (_ptr(s) if s.size else None, s.size, _ptr(t) if t.size else None, t.size, _ptr(p) if p.size else None, p.size)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _host(a, dtype, n=None, name="array"):
    a = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and a.size != n:
        raise ValueError("%s has %d elements, expected %d" % (name, a.size, n))
    return a


class Context:
    """One ptmi_ctx.  Methods map 1:1 onto include/ptmi.h."""

    def __init__(self, device=0, library=None):
        self._lib = library if library is not None else load_library()
        h = _vp()
        rc = self._lib.ptmi_create(C.byref(h), int(device))
        if rc != PTMI_OK:
            raise PtmiError(rc, (self._lib.ptmi_last_error(None) or b"").decode())
        self._h = h
        self.width = self.height = 0
        self._keep = []   # keeps bound tensors alive

    # -- plumbing --------------------------------------------------------------------
    def _check(self, rc):
        if rc != PTMI_OK:
            raise PtmiError(rc, (self._lib.ptmi_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ptmi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ---------------------------------------------------------------
    def set_scene(self, spheres, planes):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE)
        self._check(self._lib.ptmi_set_scene(self._h, _ptr(s) if s.size else None, s.size,
                                             _ptr(p) if p.size else None, p.size))

    def set_scene_bvh(self, spheres, planes):
        """ptmi_set_scene_bvh: the same scene semantics, the spheres through a bounding-volume hierarchy (up to MAX_BVH_SPHERES)."""
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE)
        self._check(self._lib.ptmi_set_scene_bvh(self._h, _ptr(s) if s.size else None, s.size,
                                                 _ptr(p) if p.size else None, p.size))

    def set_scene_mesh(self, spheres, triangles, planes):
        """ptmi_set_scene_mesh: spheres and planes as set_scene_bvh, plus triangles (TRIANGLE_DTYPE, up to MAX_MESH_TRIANGLES) through a
        second hierarchy; triangle k is primitive len(spheres) + len(planes) + k."""
        keep, args = _mesh_args(spheres, triangles, planes)
        self._check(self._lib.ptmi_set_scene_mesh(self._h, *args))
        del keep

    def update_mesh_vertices(self, v):
        """ptmi_update_mesh_vertices: move the mesh scene's vertices and refit its hierarchy on the device.  v: (n, 3, 3) or (n, 9)
        float32, v0 v1 v2 per triangle in set_scene_mesh's index order -- a numpy array (host entry), or an object with is_cuda and
        data_ptr() such as a contiguous float32 torch tensor on the context's device (device entry; the caller orders its writes
        before the context's stream)."""
        if hasattr(v, "is_cuda") and hasattr(v, "data_ptr"):
            ptr, n = _device_vertices(v)
            self._check(self._lib.ptmi_update_mesh_vertices_device(self._h, ptr, n))
        else:
            a, n = _vertex_array(v)
            self._check(self._lib.ptmi_update_mesh_vertices(self._h, _ptr(a) if n else None, n))

    def set_mesh_triangles(self, triangles):
        """ptmi_set_mesh_triangles: replace the mesh scene's triangles (any count) and build their hierarchy on the device.  triangles:
        what set_scene_mesh accepts (host entry), or an object with is_cuda and data_ptr() such as a contiguous float32 torch tensor of
        shape [n, 15] on the context's device, brdf_tag as its int32 bit pattern (device entry; the caller orders its writes before the
        context's stream)."""
        if hasattr(triangles, "is_cuda") and hasattr(triangles, "data_ptr"):
            ptr, n = _device_triangles(triangles)
            self._check(self._lib.ptmi_set_mesh_triangles_device(self._h, ptr, n))
        else:
            t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
            self._check(self._lib.ptmi_set_mesh_triangles(self._h, _ptr(t) if t.size else None, t.size))

    def update_spheres(self, g):
        """ptmi_update_spheres: move the spheres of a BVH or mesh scene and refit their hierarchy on the device.  g: (n, 4) float32 --
        x, y, z, radius in the scene's index order -- a numpy array (host entry), or an object with is_cuda and data_ptr() such as a
        contiguous float32 torch tensor on the context's device (device entry; the caller orders its writes before the context's
        stream, and keeps the tensor until the stream has passed the call)."""
        if hasattr(g, "is_cuda") and hasattr(g, "data_ptr"):
            ptr, n = _device_rows(g, 4, "sphere geometry")
            self._check(self._lib.ptmi_update_spheres_device(self._h, ptr if n else None, n))
        else:
            a = np.ascontiguousarray(g, dtype=np.float32)
            if a.size % 4 or (a.size and (a.ndim != 2 or a.shape[1] != 4)):
                raise ValueError("sphere geometry must have shape (n, 4), not %r" % (a.shape,))
            self._check(self._lib.ptmi_update_spheres(self._h, _ptr(a) if a.size else None, a.size // 4))

    def set_bvh_spheres(self, spheres):
        """ptmi_set_bvh_spheres: replace the spheres of a BVH or mesh scene (any count) and build their hierarchy on the device.  spheres:
        what set_scene_bvh accepts (host entry), or an object with is_cuda and data_ptr() such as a contiguous float32 torch tensor of
        shape [n, 10] on the context's device, brdf_tag as its int32 bit pattern in word 8 (device entry)."""
        if hasattr(spheres, "is_cuda") and hasattr(spheres, "data_ptr"):
            ptr, n = _device_rows(spheres, 10, "spheres")
            self._check(self._lib.ptmi_set_bvh_spheres_device(self._h, ptr if n else None, n))
        else:
            s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
            self._check(self._lib.ptmi_set_bvh_spheres(self._h, _ptr(s) if s.size else None, s.size))

    def bvh_read_layout(self):
        """ptmi_bvh_read_layout: the sphere hierarchy the device holds now -> (nodes, order), as bvh_layout returns them"""
        n_nodes = self._lib.ptmi_bvh_read_layout(self._h, None, 0, None)      # (nothing copied: the size)
        if n_nodes < 0:
            self._check(n_nodes)
        nodes = np.zeros(n_nodes, BVH_NODE_DTYPE)
        got = self._lib.ptmi_bvh_read_layout(self._h, _ptr(nodes), nodes.size, None)      # (the nodes alone: their leaves say how long the order is)
        if got < 0:
            self._check(got)
        ref = nodes["ref"][:got].reshape(-1).astype(np.int64)
        n_spheres = int(np.sum((-1 - ref[ref < -1]) & 255))
        order = np.zeros(max(1, n_spheres), np.int32)
        got = self._lib.ptmi_bvh_read_layout(self._h, _ptr(nodes), nodes.size, _ptr(order))
        if got < 0:
            self._check(got)
        return nodes[:got], order[:n_spheres].copy()

    def mesh_read_layout(self):
        """ptmi_mesh_read_layout: the triangle hierarchy the device holds now -> (nodes, order), as mesh_layout returns them"""
        kept = C.c_int(0)
        n_nodes = self._lib.ptmi_mesh_read_layout(self._h, None, 0, None, C.byref(kept))      # (nothing copied: the sizes)
        if n_nodes < 0:
            self._check(n_nodes)
        nodes, order = np.zeros(n_nodes, BVH_NODE_DTYPE), np.zeros(max(1, kept.value), np.int32)
        got = self._lib.ptmi_mesh_read_layout(self._h, _ptr(nodes), nodes.size, _ptr(order), C.byref(kept))
        if got < 0:
            self._check(got)
        return nodes[:got], order[:kept.value].copy()

    def set_partition(self, stripe_rows, n_parts, part):
        self._check(self._lib.ptmi_set_partition(self._h, stripe_rows, n_parts, part))

    def resize(self, width, height):
        self._check(self._lib.ptmi_resize(self._h, width, height))
        self.width, self.height = width, height
        self._keep = []

    @property
    def local_rows(self):
        rc = self._lib.ptmi_local_rows(self._h)
        if rc < 0:
            self._check(rc)
        return rc

    def global_row(self, local_row):
        rc = self._lib.ptmi_global_row(self._h, local_row)
        if rc < 0:
            raise PtmiError(rc, "ptmi_global_row")
        return rc

    def global_rows(self):
        return np.array([self.global_row(i) for i in range(self.local_rows)], dtype=np.int64)

    @property
    def n_local(self):
        return self.local_rows * self.width

    def bind_torch(self, color, state):
        """color: float32 CUDA tensor [3, rows, W]; state: int32 CUDA tensor [4, rows, W] (uint32 bits)."""
        assert color.is_cuda and state.is_cuda and color.is_contiguous() and state.is_contiguous()
        assert tuple(color.shape) == (3, self.local_rows, self.width), color.shape
        assert tuple(state.shape) == (4, self.local_rows, self.width), state.shape
        assert color.element_size() == 4 and state.element_size() == 4
        self.bind_planes([color[i].data_ptr() for i in range(3)] + [state[i].data_ptr() for i in range(4)], keep=[color, state])

    def bind_planes(self, ptrs, keep=None):
        """ptmi_bind_planes with seven raw device addresses (ints; r g b sa sb sc sctr), each of local_rows x width 4-byte elements, 4-byte
        aligned, anywhere relative to each other.  keep: whatever owns that memory, held alive while the binding stands."""
        ptrs = list(ptrs)
        if len(ptrs) != 7:
            raise ValueError("seven plane addresses, not %d" % len(ptrs))
        self._check(self._lib.ptmi_bind_planes(self._h, *[_vp(p) if p else None for p in ptrs]))
        self._keep = [keep]

    def unbind(self):
        self._check(self._lib.ptmi_bind_planes(self._h, *([None] * 7)))
        self._keep = []

    def device_planes(self):
        """Device addresses (ints) of the seven planes the context renders into."""
        ptrs = [_vp() for _ in range(7)]
        self._check(self._lib.ptmi_get_planes(self._h, *[C.byref(p) for p in ptrs]))
        return [p.value for p in ptrs]

    def set_stream(self, hip_stream):
        self._check(self._lib.ptmi_set_stream(self._h, _vp(hip_stream) if hip_stream else None))

    def set_timing(self, enabled):
        self._check(self._lib.ptmi_set_timing(self._h, int(bool(enabled))))

    def set_variant(self, variant):
        self._check(self._lib.ptmi_set_variant(self._h, int(variant)))

    def set_option(self, option, value):
        self._check(self._lib.ptmi_set_option(self._h, int(option), C.c_int64(int(value))))

    def get_option(self, option):
        v = C.c_int64(0)
        self._check(self._lib.ptmi_get_option(self._h, int(option), C.byref(v)))
        return int(v.value)

    # -- state -----------------------------------------------------------------------
    def init_output(self, seed0):
        self._check(self._lib.ptmi_init_output(self._h, C.c_uint64(seed0)))

    def reseed(self, seed0):
        self._check(self._lib.ptmi_reseed(self._h, C.c_uint64(seed0)))

    def create_with(self, w0, w1, w2):
        n = self.n_local
        ws = [_host(w, np.uint32, n, "word plane") for w in (w0, w1, w2)]
        self._check(self._lib.ptmi_create_with(self._h, *[_ptr(w) for w in ws]))

    def upload_state(self, r=None, g=None, b=None, sa=None, sb=None, sc=None, sctr=None):
        n = self.n_local
        arrs = [None if a is None else _host(a, np.float32, n) for a in (r, g, b)] + \
               [None if a is None else _host(a, np.uint32, n) for a in (sa, sb, sc, sctr)]
        self._check(self._lib.ptmi_upload_state(self._h, *[_ptr(a) for a in arrs]))

    def download_state(self):
        shape = (self.local_rows, self.width)
        out = [np.empty(shape, np.float32) for _ in range(3)] + [np.empty(shape, np.uint32) for _ in range(4)]
        self._check(self._lib.ptmi_download_state(self._h, *[_ptr(a) for a in out]))
        return tuple(out)

    def download_color(self):
        shape = (self.local_rows, self.width)
        out = [np.empty(shape, np.float32) for _ in range(3)]
        self._check(self._lib.ptmi_download_color(self._h, *[_ptr(a) for a in out]))
        return tuple(out)

    # -- hot path --------------------------------------------------------------------
    def render(self, camera, bounce_limit, n_spp, algorithm=INLINE):
        cam = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE)
        self._check(self._lib.ptmi_render(self._h, _ptr(cam), algorithm, bounce_limit, n_spp))

    def synchronize(self):
        self._check(self._lib.ptmi_synchronize(self._h))

    def render_blocks(self, algorithm=INLINE):
        rc = self._lib.ptmi_render_blocks(self._h, int(algorithm))
        if rc < 0:
            self._check(rc)
        return rc == 1

    def render1(self, camera, bounce_limit, width, height, planes_in, algorithm=INLINE, screen=None):
        """compileFor's closure (app/Main.hs:188-191): 7 host planes in -> 7 new host planes out."""
        cam = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE)
        n = width * height
        ins = [_host(a, np.float32, n) for a in planes_in[:3]] + [_host(a, np.uint32, n) for a in planes_in[3:]]
        outs = [np.empty((height, width), np.float32) for _ in range(3)] + \
               [np.empty((height, width), np.uint32) for _ in range(4)]
        sx = sy = None
        if screen is not None:
            sx, sy = _host(screen[0], np.int64, n), _host(screen[1], np.int64, n)
        self._check(self._lib.ptmi_render1(self._h, _ptr(cam), algorithm, bounce_limit, width, height,
                                           _ptr(sx), _ptr(sy), *[_ptr(a) for a in ins], *[_ptr(a) for a in outs]))
        return tuple(outs)

    # -- the closure, chained (device residency behind compileFor's pure type) ----------
    def render1_chained(self, camera, bounce_limit, width, height, token=0, planes_in=None, algorithm=INLINE, consume=False, fetch=()):
        """One application of the closure to the state `token` names (or, if the context does not hold it, to the seven host planes
        planes_in).  Returns (new token, {plane name: array} for the names in `fetch`, a subset of r g b sa sb sc sctr)."""
        cam = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE)
        n = width * height
        ins = [None] * 7
        if planes_in is not None:
            ins = [_host(a, np.float32, n) for a in planes_in[:3]] + [_host(a, np.uint32, n) for a in planes_in[3:]]
        names = "r g b sa sb sc sctr".split()
        outs = [np.empty((height, width), np.float32 if i < 3 else np.uint32) if names[i] in fetch else None for i in range(7)]
        tok = C.c_uint64(0)
        self._check(self._lib.ptmi_render1_chained(self._h, _ptr(cam), algorithm, bounce_limit, width, height, C.c_uint64(int(token)),
                                                   CHAIN_CONSUME if consume else 0, *[_ptr(a) for a in ins], C.byref(tok), *[_ptr(a) for a in outs]))
        return int(tok.value), {nm: a for nm, a in zip(names, outs) if a is not None}

    def chain_init_output(self, width, height, seed0):
        tok = C.c_uint64(0)
        self._check(self._lib.ptmi_chain_init_output(self._h, width, height, C.c_uint64(seed0), C.byref(tok)))
        return int(tok.value)

    def chain_reseed(self, seed0, width, height, token=0, colour_in=None, consume=False):
        ins = [None] * 3 if colour_in is None else [_host(a, np.float32, width * height) for a in colour_in]
        tok = C.c_uint64(0)
        self._check(self._lib.ptmi_chain_reseed(self._h, C.c_uint64(seed0), width, height, C.c_uint64(int(token)), CHAIN_CONSUME if consume else 0,
                                                *[_ptr(a) for a in ins], C.byref(tok)))
        return int(tok.value)

    def chain_fetch(self, token, width, height, planes="r g b sa sb sc sctr"):
        names = "r g b sa sb sc sctr".split()
        want = planes.split() if isinstance(planes, str) else list(planes)
        outs = [np.empty((height, width), np.float32 if i < 3 else np.uint32) if names[i] in want else None for i in range(7)]
        self._check(self._lib.ptmi_chain_fetch(self._h, C.c_uint64(int(token)), *[_ptr(a) for a in outs]))
        return tuple(a for a in outs if a is not None)

    def chain_release(self, token):
        self._check(self._lib.ptmi_chain_release(self._h, C.c_uint64(int(token))))

    def chain_info(self):
        st = ChainStats()
        self._check(self._lib.ptmi_chain_info(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in ChainStats._fields_}

    def present(self, iterations, rgb32f=True, rgba8=True):
        """graphicsLoop + fs.glsl: interleaved colour / iterations as float RGB and/or 8-bit RGBA."""
        shape = (self.local_rows, self.width)
        rgb = np.empty(shape + (3,), np.float32) if rgb32f else None
        rgba = np.empty(shape + (4,), np.uint8) if rgba8 else None
        self._check(self._lib.ptmi_present(self._h, int(iterations), _ptr(rgb), _ptr(rgba)))
        return rgb, rgba

    def stats(self):
        st = Stats()
        self._check(self._lib.ptmi_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in Stats._fields_}

    def debug_counters(self):
        out = np.zeros(256, np.uint32)
        n = self._lib.ptmi_debug_counters_n(self._h, _ptr(out), out.size)
        if n < 0:
            self._check(n)
        return out

    def reset_stats(self):
        self._check(self._lib.ptmi_reset_stats(self._h))

    # -- point queries ---------------------------------------------------------------
    def eval_distance_to_sphere(self, spheres, rays):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        r = _host(rays, np.float32, s.size * 6, "rays")
        n = s.size
        just, t, nrm = np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 6), np.float32)
        self._check(self._lib.ptmi_eval_distance_to_sphere(self._h, _ptr(s), _ptr(r), n, _ptr(just), _ptr(t), _ptr(nrm)))
        return just, t, nrm

    def eval_distance_to_plane(self, planes, rays):
        p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE)
        r = _host(rays, np.float32, p.size * 6, "rays")
        n = p.size
        just, t, nrm = np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 6), np.float32)
        self._check(self._lib.ptmi_eval_distance_to_plane(self._h, _ptr(p), _ptr(r), n, _ptr(just), _ptr(t), _ptr(nrm)))
        return just, t, nrm

    def eval_check_hit(self, rays):
        """ptmi_eval_check_hit: checkHit on the device against the current scene for rays (n x 6) -> (t, idx, just); a miss is t 0, idx -1."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        t, idx, just = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32)
        self._check(self._lib.ptmi_eval_check_hit(self._h, _ptr(r), n, _ptr(t), _ptr(idx), _ptr(just)))
        return t, idx, just

    # -- ray queries on the device ------------------------------------------------------
    def trace_rays(self, rays, hit=False, out=None, index=None):
        """ptmi_trace_rays_device: the closest hit of every ray against the current scene, on the context's stream, nothing leaving the
        device.  rays: a contiguous float32 device tensor of shape (n, 6) -- origin, direction -- anything with is_cuda and data_ptr();
        the caller orders its writes before the context's stream and keeps the tensors until the stream has passed the call (after
        set_stream(torch's stream) that stream orders both; on the context's own stream: torch.cuda.synchronize() before the call,
        synchronize() before the results are read).
        -> (t, idx), or (t, idx, hit) with hit=True: t float32 (n,), idx int32 (n,) -- spheres, then planes, then triangles; a miss is
        t 0, idx -1 -- and hit float32 (n, 6), position and normal, zeros for a miss.  They are allocated with torch.empty on the rays'
        device unless out=(t, idx) or out=(t, idx, hit) gives the caller's own.
        index: an int32 device tensor (m,) -- ptmi_trace_rays_indexed_device: only the rays it names are traced, in its order (ray_order's,
        or a caller's list of live rays), each answer at its ray's position; an entry outside [0, n) is skipped.  Outputs allocated here
        are then filled with the miss record first (t 0, idx -1, zeros), so the positions no entry names are defined -- by torch, on its
        current stream: the context must launch on that stream (set_stream), as for any input torch writes.  A caller's out= is left as
        it is at those positions."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        if out is not None:
            if len(out) not in (2, 3):
                raise ValueError("out must be (t, idx) or (t, idx, hit)")
            hit = len(out) == 3
            outs = tuple(out)
        elif index is None:
            import torch
            outs = (torch.empty(n, dtype=torch.float32, device=rays.device), torch.empty(n, dtype=torch.int32, device=rays.device))
            if hit:
                outs += (torch.empty((n, 6), dtype=torch.float32, device=rays.device),)
        else:
            import torch
            outs = (torch.zeros(n, dtype=torch.float32, device=rays.device), torch.full((n,), -1, dtype=torch.int32, device=rays.device))
            if hit:
                outs += (torch.zeros((n, 6), dtype=torch.float32, device=rays.device),)
        d_t = _device_tensor(outs[0], "float32", (n,), "t")
        d_idx = _device_tensor(outs[1], "int32", (n,), "idx")
        d_hit = _device_tensor(outs[2], "float32", (n, 6), "hit") if hit else None
        if index is None:
            self._check(self._lib.ptmi_trace_rays_device(self._h, d_rays, n, d_t, d_idx, d_hit))
        else:
            self._check(self._lib.ptmi_trace_rays_indexed_device(self._h, d_rays, n, d_index, int(index.shape[0]), d_t, d_idx, d_hit))
        return outs

    def occluded(self, rays, t_max, out=None, index=None):
        """ptmi_occluded_device: 1 where the closest hit of a ray is nearer than its t_max, else 0 (a NaN or non-positive t_max: 0), found
        by an any-hit walk on the context's stream.  rays as trace_rays takes them, t_max a contiguous float32 device tensor of shape
        (n,) -> an int32 device tensor (n,): `out`, or one allocated with torch.empty on the rays' device.
        index: as for trace_rays (ptmi_occluded_indexed_device); an output allocated here is then filled with 0 first."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        d_t_max = _device_tensor(t_max, "float32", (n,), "t_max")
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        if out is None:
            import torch
            out = (torch.empty if index is None else torch.zeros)(n, dtype=torch.int32, device=rays.device)
        d_out = _device_tensor(out, "int32", (n,), "out")
        if index is None:
            self._check(self._lib.ptmi_occluded_device(self._h, d_rays, d_t_max, n, d_out))
        else:
            self._check(self._lib.ptmi_occluded_indexed_device(self._h, d_rays, d_t_max, n, d_index, int(index.shape[0]), d_out))
        return out

    def trace_rays_multi(self, rays, k, t_max=None, out=None, index=None):
        """ptmi_trace_rays_multi_device: the k nearest hits of every ray, in order, before its t_max (None: no limit), on the context's
        stream.  rays as trace_rays takes them, 1 <= k <= MULTI_HIT_MAX, t_max a contiguous float32 device tensor of shape (n,).
        -> (t, idx, count): t float32 (n, k) and idx int32 (n, k) -- row i the count[i] nearest hits ascending by (t, primitive), each
        primitive once, then the miss record, t 0 and idx -1 -- and count int32 (n,).  They are allocated with torch.empty on the rays'
        device unless out=(t, idx, count) gives the caller's own.
        index: as for trace_rays (ptmi_trace_rays_multi_indexed_device); outputs allocated here are then filled with the miss record and
        a count of 0 first."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MULTI_HIT_MAX:
            raise ValueError("k must be an int in [1, %d], not %r" % (MULTI_HIT_MAX, k))
        d_t_max = _device_tensor(t_max, "float32", (n,), "t_max") if t_max is not None else None
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        if out is not None:
            if len(out) != 3:
                raise ValueError("out must be (t, idx, count)")
            outs = tuple(out)
        else:
            import torch
            if index is None:
                outs = (torch.empty((n, k), dtype=torch.float32, device=rays.device), torch.empty((n, k), dtype=torch.int32, device=rays.device),
                        torch.empty(n, dtype=torch.int32, device=rays.device))
            else:
                outs = (torch.zeros((n, k), dtype=torch.float32, device=rays.device), torch.full((n, k), -1, dtype=torch.int32, device=rays.device),
                        torch.zeros(n, dtype=torch.int32, device=rays.device))
        d_t = _device_tensor(outs[0], "float32", (n, k), "t")
        d_idx = _device_tensor(outs[1], "int32", (n, k), "idx")
        d_count = _device_tensor(outs[2], "int32", (n,), "count")
        if index is None:
            self._check(self._lib.ptmi_trace_rays_multi_device(self._h, d_rays, d_t_max, n, k, d_t, d_idx, d_count))
        else:
            self._check(self._lib.ptmi_trace_rays_multi_indexed_device(self._h, d_rays, d_t_max, n, d_index, int(index.shape[0]), k, d_t, d_idx, d_count))
        return outs

    def nearest(self, points, r_max=None, point=False, out=None, index=None):
        """ptmi_nearest_device: the nearest-primitive query -- for every point the primitive of the current scene with the least
        (|signed distance|, index) within its r_max (None: no limit), on the context's stream, nothing leaving the device.  points: a
        contiguous float32 device tensor of shape (n, 3), r_max one of shape (n,); ordering and lifetime as for trace_rays.
        -> (dist, idx), or (dist, idx, point) with point=True: dist float32 (n,), the signed distance, negative behind the surface; idx
        int32 (n,) -- spheres, then planes, then triangles; a miss is dist 0, idx -1, location (0, 0, 0) -- and point float32 (n, 3), the
        nearest location on the primitive.  They are allocated with torch.empty on the points' device unless out=(dist, idx) or
        out=(dist, idx, point) gives the caller's own.
        index: as for trace_rays (ptmi_nearest_indexed_device); outputs allocated here are then filled with the miss record first."""
        d_points = _device_tensor(points, "float32", (None, 3), "points")
        n = int(points.shape[0])
        d_r_max = _device_tensor(r_max, "float32", (n,), "r_max") if r_max is not None else None
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        if out is not None:
            if len(out) not in (2, 3):
                raise ValueError("out must be (dist, idx) or (dist, idx, point)")
            point = len(out) == 3
            outs = tuple(out)
        else:
            import torch
            if index is None:
                outs = (torch.empty(n, dtype=torch.float32, device=points.device), torch.empty(n, dtype=torch.int32, device=points.device))
                if point:
                    outs += (torch.empty((n, 3), dtype=torch.float32, device=points.device),)
            else:
                outs = (torch.zeros(n, dtype=torch.float32, device=points.device), torch.full((n,), -1, dtype=torch.int32, device=points.device))
                if point:
                    outs += (torch.zeros((n, 3), dtype=torch.float32, device=points.device),)
        d_dist = _device_tensor(outs[0], "float32", (n,), "dist")
        d_idx = _device_tensor(outs[1], "int32", (n,), "idx")
        d_at = _device_tensor(outs[2], "float32", (n, 3), "point") if point else None
        if index is None:
            self._check(self._lib.ptmi_nearest_device(self._h, d_points, d_r_max, n, d_dist, d_idx, d_at))
        else:
            self._check(self._lib.ptmi_nearest_indexed_device(self._h, d_points, d_r_max, n, d_index, int(index.shape[0]), d_dist, d_idx, d_at))
        return outs

    def ray_order(self, rays, out=None, work=None):
        """ptmi_ray_order_device: a coherent order for the batch, on the context's stream, nothing leaving the device -> an int32 device
        tensor (n,): the ray of every position, ascending by (key, index) -- the index= of trace_rays / occluded.  No scene is needed.
        out: the caller's own int32 (n,); work: a uint8 device tensor of at least ray_order_bytes(n) elements, 8-byte aligned, scratch
        while the call is in flight.  Both are allocated with torch.empty on the rays' device by default; a workspace allocated here
        goes back to torch's allocator when this returns, which is safe when the context launches on torch's current stream
        (set_stream) -- otherwise give work= and keep it until the stream has passed the call."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        need = int(self._lib.ptmi_ray_order_bytes(n))
        if out is None or work is None:
            import torch
            if out is None:
                out = torch.empty(n, dtype=torch.int32, device=rays.device)
            if work is None:
                work = torch.empty(need, dtype=torch.uint8, device=rays.device)
        d_out = _device_tensor(out, "int32", (n,), "out")
        d_work = _device_tensor(work, "uint8", (None,), "work")
        if int(work.shape[0]) < need:
            raise ValueError("work must hold ray_order_bytes(n) = %d bytes, not %d" % (need, int(work.shape[0])))
        self._check(self._lib.ptmi_ray_order_device(self._h, d_rays, n, d_out, d_work, int(work.shape[0])))
        return out

    # -- paths along a caller's rays ------------------------------------------------------
    @staticmethod
    def _seed_tensor(t, n, what):
        """seeds: a contiguous device tensor (n, 4) of any 4-byte integer dtype -> its pointer"""
        name = str(getattr(t, "dtype", "")).split(".")[-1]
        return _device_tensor(t, name if name in ("int32", "uint32") else "int32", (n, 4), what)

    def path_seeds(self, seed0, n, first_index=0, out=None):
        """ptmi_path_seeds_device: the SFC32 states init_output(seed0) gives pixels first_index .. first_index + n - 1 of an unpartitioned
        image, on the context's stream -> a device tensor (n, 4): a, b, c, counter per ray -- `out` (any 4-byte integer dtype), or an int32
        one allocated with torch.empty on torch's current device.  No scene is needed."""
        n = int(n)
        if n < 0 or int(first_index) < 0:
            raise ValueError("n and first_index must not be negative")
        if out is None:
            import torch
            out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        d_out = self._seed_tensor(out, n, "out")
        self._check(self._lib.ptmi_path_seeds_device(self._h, int(seed0) & (2 ** 64 - 1), int(first_index), n, d_out))
        return out

    def trace_paths(self, rays, seeds, bounce_limit, spp=1, color=None, index=None):
        """ptmi_trace_paths_device: render Inline along the caller's rays, on the context's stream, nothing leaving the device -- for ray i,
        spp times: (new, seed') = traceInline bounce_limit scene ray_i seed_i; color_i = new + color_i; seed_i = seed'.  rays as trace_rays
        takes them (a direction of any length); seeds: a contiguous device tensor (n, 4) of any 4-byte integer dtype (path_seeds makes
        one), advanced in place; color: a contiguous float32 device tensor (n, 3), accumulated into -- allocated with torch.zeros on the rays'
        device when not given (by torch, on its current stream: the context must then launch on that stream, set_stream).  -> color.
        index: an int32 device tensor (m,) -- ptmi_trace_paths_indexed_device: only the rays it names are traced, in its order; an entry
        outside [0, n) is skipped, a ray no entry names keeps its colour and seed.  It must name a ray at most once: colour and seed are
        read and written, a ray named twice is a race."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        d_seed = self._seed_tensor(seeds, n, "seeds")
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        if color is None:
            import torch
            color = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
        d_color = _device_tensor(color, "float32", (n, 3), "color")
        if index is None:
            self._check(self._lib.ptmi_trace_paths_device(self._h, d_rays, n, int(bounce_limit), int(spp), d_color, d_seed))
        else:
            self._check(self._lib.ptmi_trace_paths_indexed_device(self._h, d_rays, n, d_index, int(index.shape[0]), int(bounce_limit), int(spp), d_color, d_seed))
        return color

    # -- stepped paths: one bounce at a time, and the live rays ----------------------------
    def bounce_rays(self, rays, seeds, throughput, radiance, index=None, hit=False, out=None):
        """ptmi_bounce_rays_device: one prepareRay for every ray, on the context's stream, nothing leaving the device.  rays (n, 6) float32,
        seeds (n, 4) of any 4-byte integer dtype, throughput and radiance (n, 3) float32: contiguous device tensors, all CHANGED IN PLACE --
        a ray whose throughput is nearZero or that hits nothing gets throughput 0 and keeps ray, radiance and seed; a ray that hits gets
        radiance += emittance * throughput, throughput *= tmod, the next ray and the advanced seed.  From throughput 1 and radiance 0,
        k calls are trace_paths(bounce_limit=k) bit for bit.
        -> None, or (t, idx, hit) -- trace_rays' words for the INCOMING rays, the miss record (0, -1, zeros) where a ray missed or was not
        traced -- with hit=True (allocated on the rays' device) or out=(t, idx, hit), the caller's own, any of the three None.
        index: an int32 device tensor (m,) -- ptmi_bounce_rays_indexed_device: only the rays it names are stepped (ray_order's order, or
        live_rays' padded list), each AT MOST ONCE; an entry outside [0, n) is skipped.  Outputs allocated here are then filled with the
        miss record first, by torch on its current stream, as for trace_rays; a caller's out= is left as it is at the other positions."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        d_seed = self._seed_tensor(seeds, n, "seeds")
        d_throughput = _device_tensor(throughput, "float32", (n, 3), "throughput")
        d_radiance = _device_tensor(radiance, "float32", (n, 3), "radiance")
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        outs = None
        if out is not None:
            if len(out) != 3:
                raise ValueError("out must be (t, idx, hit), any of them None")
            outs = tuple(out)
        elif hit:
            import torch
            if index is None:
                outs = (torch.empty(n, dtype=torch.float32, device=rays.device), torch.empty(n, dtype=torch.int32, device=rays.device),
                        torch.empty((n, 6), dtype=torch.float32, device=rays.device))
            else:
                outs = (torch.zeros(n, dtype=torch.float32, device=rays.device), torch.full((n,), -1, dtype=torch.int32, device=rays.device),
                        torch.zeros((n, 6), dtype=torch.float32, device=rays.device))
        d_t = d_idx = d_hit = None
        if outs is not None:
            d_t = _device_tensor(outs[0], "float32", (n,), "t") if outs[0] is not None else None
            d_idx = _device_tensor(outs[1], "int32", (n,), "idx") if outs[1] is not None else None
            d_hit = _device_tensor(outs[2], "float32", (n, 6), "hit") if outs[2] is not None else None
        if index is None:
            self._check(self._lib.ptmi_bounce_rays_device(self._h, d_rays, n, d_throughput, d_radiance, d_seed, d_t, d_idx, d_hit))
        else:
            self._check(self._lib.ptmi_bounce_rays_indexed_device(self._h, d_rays, n, d_index, int(index.shape[0]), d_throughput, d_radiance, d_seed,
                                                                  d_t, d_idx, d_hit))
        return outs

    def live_rays(self, throughput, index=None, out=None, count=None, work=None):
        """ptmi_live_rays_device: the rays that are still alive, on the context's stream, nothing leaving the device -> `out`, an int32 device
        tensor with one entry per candidate: the candidates -- index's entries, or 0 .. n - 1 -- inside [0, n) whose throughput (n, 3) is
        not nearZero, in candidate order, then -1: the index= of bounce_rays, trace_rays, occluded and trace_paths, with no host wait.
        out may be `index` itself (in place); count: an int32 device tensor (1,) that receives the number of live rays; work: a uint8
        device tensor of at least live_rays_bytes(candidates) elements, 8-byte aligned, scratch while the call is in flight.  out and work
        are allocated with torch.empty on the throughput's device by default, as ray_order's are.  No scene is needed."""
        d_throughput = _device_tensor(throughput, "float32", (None, 3), "throughput")
        n = int(throughput.shape[0])
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        m = int(index.shape[0]) if index is not None else 0
        candidates = m if index is not None else n
        d_count = _device_tensor(count, "int32", (1,), "count") if count is not None else None
        if out is not None:
            _device_tensor(out, "int32", (candidates,), "out")
        if work is not None:
            _device_tensor(work, "uint8", (None,), "work")
        need = int(self._lib.ptmi_live_rays_bytes(candidates))
        if out is None or work is None:
            import torch
            if out is None:
                out = torch.empty(candidates, dtype=torch.int32, device=throughput.device)
            if work is None:
                work = torch.empty(need, dtype=torch.uint8, device=throughput.device)
        d_out = _device_tensor(out, "int32", (candidates,), "out")
        d_work = _device_tensor(work, "uint8", (None,), "work")
        if int(work.shape[0]) < need:
            raise ValueError("work must hold live_rays_bytes(%d) = %d bytes, not %d" % (candidates, need, int(work.shape[0])))
        if candidates == 0:                              # (an empty index has no pointer, and a NULL index means every ray)
            return out
        self._check(self._lib.ptmi_live_rays_device(self._h, d_throughput, n, d_index, m, d_out, d_count, d_work, int(work.shape[0])))
        return out

    # -- render Streams along a caller's rays -----------------------------------------------
    def trace_streams_bytes(self, count):
        """ptmi_trace_streams_bytes: the workspace trace_streams needs for that many lanes on a scene with GLASS."""
        return int(self._lib.ptmi_trace_streams_bytes(int(count)))

    def trace_streams(self, rays, seeds, spp=1, color=None, index=None, lost=None, work=None):
        """ptmi_trace_streams_device: render Streams along the caller's rays, on the context's stream, nothing leaving the device -- for ray
        i, spp times, the sample's ray tree is walked depth first from ray_i with seed_i: every hit adds emittance * throughput to color_i,
        a GLASS hit splits the ray, no bounce limit (nearZero, a miss or OPT_STREAM_STEP_CAP ends a lineage), the seed rule of
        OPT_STREAMS_SEED_RULE; then seed_i advances one draw.  rays, seeds, color and index as trace_paths takes them; -> color.
        lost: an int64 device tensor (2,), ADDED to: the rays the step cap cut and the children a full stack dropped.
        work: a uint8 device tensor of at least trace_streams_bytes(lanes) elements, 16-byte aligned, scratch while the call is in flight
        (lanes: the index's length, or n); only a scene with GLASS uses it.  The binding cannot see whether the scene holds GLASS, so it
        allocates one with torch.empty on the rays' device when none is given and keeps it for later calls."""
        d_rays = _device_tensor(rays, "float32", (None, 6), "rays")
        n = int(rays.shape[0])
        d_seed = self._seed_tensor(seeds, n, "seeds")
        d_index = _device_tensor(index, "int32", (None,), "index") if index is not None else None
        d_lost = _device_tensor(lost, "int64", (2,), "lost") if lost is not None else None
        if work is not None:
            _device_tensor(work, "uint8", (None,), "work")
        if color is None:
            import torch
            color = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
        d_color = _device_tensor(color, "float32", (n, 3), "color")
        lanes = int(index.shape[0]) if index is not None else n
        if lanes == 0 or n == 0 or int(spp) <= 0:       # (an empty index has no pointer, and nothing would be touched)
            return color
        if work is None:
            need = self.trace_streams_bytes(lanes)
            work = getattr(self, "_streams_work", None)
            if work is None or int(work.shape[0]) < need or work.device != rays.device:
                import torch
                work = self._streams_work = torch.empty(need, dtype=torch.uint8, device=rays.device)
        d_work = _device_tensor(work, "uint8", (None,), "work")
        if index is None:
            self._check(self._lib.ptmi_trace_streams_device(self._h, d_rays, n, int(spp), d_color, d_seed, d_lost, d_work, int(work.shape[0])))
        else:
            self._check(self._lib.ptmi_trace_streams_indexed_device(self._h, d_rays, n, d_index, lanes, int(spp), d_color, d_seed, d_lost, d_work,
                                                                    int(work.shape[0])))
        return color

    def eval_sincos(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        s, c = np.empty_like(x), np.empty_like(x)
        self._check(self._lib.ptmi_eval_sincos(self._h, _ptr(x), x.size, _ptr(s), _ptr(c)))
        return s, c

    def eval_quaternion(self, half_angles):
        """ptmi_eval_quaternion: quaternion_from_half_angles on the device for half angles (n x 3) -> (n x 4: w, x, y, z); rows 64 k .. 64 k + 63 share a wave."""
        a = np.ascontiguousarray(half_angles, dtype=np.float32).reshape(-1, 3)
        q = np.empty((a.shape[0], 4), np.float32)
        self._check(self._lib.ptmi_eval_quaternion(self._h, _ptr(a), a.shape[0], _ptr(q)))
        return q


class Group:
    """One ptmi_group: the GPUs of a node behind one host process (include/ptmi.h, "groups")."""

    def __init__(self, devices, stripe_rows=0, library=None):
        self._lib = library if library is not None else load_library()
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = _vp()
        rc = self._lib.ptmi_group_create(C.byref(h), devs.ctypes.data_as(_i32p), devs.size, int(stripe_rows))
        if rc != PTMI_OK:
            raise PtmiError(rc, (self._lib.ptmi_last_error(None) or b"").decode())
        self._h = h
        self.width = self.height = 0

    def _check(self, rc):
        if rc != PTMI_OK:
            raise PtmiError(rc, (self._lib.ptmi_group_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ptmi_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return self._lib.ptmi_group_size(self._h)

    def member(self, i):
        """A non-owning Context view of member i (do not close it)."""
        c = Context.__new__(Context)
        c._lib, c._h, c._keep = self._lib, _vp(self._lib.ptmi_group_member(self._h, i)), []
        c.width, c.height = self.width, self.height
        c.close = lambda: None
        return c

    def set_scene(self, spheres, planes):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE)
        self._check(self._lib.ptmi_group_set_scene(self._h, _ptr(s) if s.size else None, s.size, _ptr(p) if p.size else None, p.size))

    def set_scene_bvh(self, spheres, planes):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, dtype=PLANE_DTYPE)
        self._check(self._lib.ptmi_group_set_scene_bvh(self._h, _ptr(s) if s.size else None, s.size, _ptr(p) if p.size else None, p.size))

    def update_mesh_vertices(self, v):
        """ptmi_group_update_mesh_vertices: Context.update_mesh_vertices (host memory) on every member"""
        a, n = _vertex_array(v)
        self._check(self._lib.ptmi_group_update_mesh_vertices(self._h, _ptr(a) if n else None, n))

    def set_mesh_triangles(self, triangles):
        """ptmi_group_set_mesh_triangles: Context.set_mesh_triangles (host memory) on every member"""
        t = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
        self._check(self._lib.ptmi_group_set_mesh_triangles(self._h, _ptr(t) if t.size else None, t.size))

    def update_spheres(self, g):
        a = np.ascontiguousarray(g, dtype=np.float32)
        if a.size % 4 or (a.size and (a.ndim != 2 or a.shape[1] != 4)):
            raise ValueError("sphere geometry must have shape (n, 4), not %r" % (a.shape,))
        self._check(self._lib.ptmi_group_update_spheres(self._h, _ptr(a) if a.size else None, a.size // 4))

    def set_bvh_spheres(self, spheres):
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
        self._check(self._lib.ptmi_group_set_bvh_spheres(self._h, _ptr(s) if s.size else None, s.size))

    def set_scene_mesh(self, spheres, triangles, planes):
        keep, args = _mesh_args(spheres, triangles, planes)
        self._check(self._lib.ptmi_group_set_scene_mesh(self._h, *args))
        del keep

    def resize(self, width, height):
        self._check(self._lib.ptmi_group_resize(self._h, width, height))
        self.width, self.height = width, height

    def init_output(self, seed0):
        self._check(self._lib.ptmi_group_init_output(self._h, C.c_uint64(seed0)))

    def reseed(self, seed0):
        self._check(self._lib.ptmi_group_reseed(self._h, C.c_uint64(seed0)))

    def render(self, camera, bounce_limit, n_spp, algorithm=INLINE):
        cam = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE)
        self._check(self._lib.ptmi_group_render(self._h, _ptr(cam), algorithm, bounce_limit, n_spp))

    def set_option(self, option, value):
        self._check(self._lib.ptmi_group_set_option(self._h, int(option), C.c_int64(int(value))))

    def set_variant(self, variant):
        self._check(self._lib.ptmi_group_set_variant(self._h, int(variant)))

    def synchronize(self):
        self._check(self._lib.ptmi_group_synchronize(self._h))

    def download_color(self):
        out = [np.empty((self.height, self.width), np.float32) for _ in range(3)]
        self._check(self._lib.ptmi_group_download_color(self._h, *[_ptr(a) for a in out]))
        return tuple(out)

    def gather_color(self, root, r_dev, g_dev, b_dev):
        """r_dev, g_dev, b_dev: device pointers (int) of [height][width] float planes on member `root`'s device."""
        self._check(self._lib.ptmi_group_gather_color(self._h, int(root), _vp(r_dev), _vp(g_dev), _vp(b_dev)))

    def stats(self):
        st = Stats()
        self._check(self._lib.ptmi_group_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in Stats._fields_}
