"""Python wrappers of libloftr_global.so (include/loftr_global.h): global positioning (csrc/position.hip, csrc/position_gpu.hip;
DESIGN §27).  The two sides of the routine share one body, written against the backends of ``ops`` (``_Host`` on numpy arrays defines
the result, ``_Gpu`` on GPU tensors reproduces it); the second library is loaded lazily, on the first call."""
from . import _lib
from .ops import _Gpu, _Host, _StageMs, _check_args, _on_device, _outputs, _stream

POSITION_COUNTS = 16
POSITION_NAMES = ("n_trials", "error_bits", "n_accepted", "n_pcg_iters", "n_active_obs", "n_active_points", "n_free", "n_negative_scale",
                  "n_tree_no_direction", "status", "tree_depth", "n_in_graph", "n_chained")                  # counts[0..12]
POSITION_INFO = ("cost_start", "cost_end", "lambda", "last_step")                         # info[0..3]
POSITION_STATUS = ("converged", "max_iters", "stalled", "nothing")                        # counts[9]
POSITION_CAM_STATES = ("outside", "chained_only", "solved", "root")                       # cam_state codes 0..3
POSITION_OBS_STATES = ("unused", "active", "negative_scale")                              # obs_state codes 0..2
POSITION_STAGES = ("check", "start", "setup", "refine", "write")
POSITION_ERRORS = ((1, "obs_image outside [0, n_images)"), (2, "offsets must start at 0, end at N and ascend"),
                   (4, "cam_offsets / cam_obs must group the observations by image in ascending order"),
                   (8, "root outside [0, n_images) or outside the graph"),
                   (16, "a tree edge outside the graph, or a tree that is not a tree rooted at root"))   # bits of counts[1]
_POS_ARGS = (("offsets", "int64", 1), ("obs_image", "int32", 1), ("obs_xy", "float32", 2), ("cam_offsets", "int64", 1),
             ("cam_obs", "int32", 1), ("K", "float64", 3), ("R", "float64", 3), ("in_graph", "uint8", 1), ("tree_image", "int32", 2),
             ("tree_t", "float64", 2))
_POS_OUT = (("centres", "n", (3,), "float64"), ("xyz", "T", (3,), "float32"), ("depth_scale", "N", (), "float64"),
            ("obs_state", "N", (), "uint8"), ("cam_state", "n", (), "uint8"), ("point_active", "T", (), "uint8"))


def _global_positions(B, what, hint, arrays, root, huber, max_iters, pcg_iters, pcg_tol, ftol, min_cam_obs, timings):
    from . import _lib_global
    _check_args(B, what, hint, _POS_ARGS, arrays)
    offsets, obs_image, obs_xy, cam_offsets, cam_obs, K, R, in_graph, tree_image, tree_t = arrays
    T, N, n, Et = offsets.shape[0] - 1, obs_image.shape[0], in_graph.shape[0], tree_image.shape[0]
    for name, v, lo in (("root", root, -(1 << 31)), ("max_iters", max_iters, 0), ("pcg_iters", pcg_iters, 0), ("min_cam_obs", min_cam_obs, 0)):
        if not isinstance(v, int) or isinstance(v, bool) or v < lo:
            raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v}")
    if (T < 0 or n < 1 or tuple(obs_xy.shape) != (N, 2) or cam_offsets.shape[0] != n + 1 or cam_obs.shape[0] != N or tuple(K.shape) != (n, 3, 3)
            or tuple(R.shape) != (n, 3, 3) or tuple(tree_image.shape) != (Et, 2) or tuple(tree_t.shape) != (Et, 3) or (T == 0 and N > 0)):
        raise _lib.LoftrHipError(f"{what}: expected offsets [T+1], obs_image [N], obs_xy [N,2], cam_offsets [n+1], cam_obs [N], K [n,3,3], "
                                 f"R [n,3,3], in_graph [n] with n >= 1, tree_image [Et,2] and tree_t [Et,3], got "
                                 f"{[tuple(a.shape) for a in arrays]}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _POS_OUT, {"n": n, "T": T, "N": N}, POSITION_COUNTS, offsets)
    out["info"] = B.zeros(len(POSITION_INFO), "float64", offsets)
    args = (a[0], T, a[1], a[2], N, a[3], a[4], a[5], a[6], a[7], n, root, a[8], a[9], Et, float(huber), max_iters, pcg_iters,
            float(pcg_tol), float(ftol), min_cam_obs, *[B.ptr(out[k]) for k in out])
    lib = _lib_global.load()
    if B is _Host:
        status = lib.loftr_global_positions_host(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad input is reported through counts[1], as on the GPU
            _lib_global.check(status, "loftr_global_positions_host")
        return out
    import torch
    ms = _StageMs(timings, POSITION_STAGES)
    buf = torch.empty(max(1, lib.loftr_global_positions_workspace_bytes(T, N, n, Et)), dtype=torch.uint8, device=offsets.device)
    _lib_global.check(lib.loftr_global_positions(*args, B.ptr(buf), buf.numel(), ms.arg, _stream()), "loftr_global_positions")
    ms.report()
    return out


def global_positions_host(offsets, obs_image, obs_xy, cam_offsets, cam_obs, K, R, in_graph, tree_image, tree_t, root, huber=0.1, max_iters=50,
                          pcg_iters=30, pcg_tol=1e-2, ftol=1e-7, min_cam_obs=8):
    """loftr_global_positions_host: the host routine that DEFINES global positioning (include/loftr_global.h) on numpy
    arrays: offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32, cam_offsets [n+1] i64, cam_obs [N] i32, K [n,3,3] f64, R [n,3,3] f64,
    in_graph [n] u8, tree_image [Et,2] i32, tree_t [Et,3] f64.
    -> dict of numpy arrays: centres [n,3] f64, xyz [T,3] f32, depth_scale [N] f64, obs_state [N] u8, cam_state [n] u8, point_active [T]
    u8, counts [16] i64 (POSITION_NAMES), info [4] f64 (POSITION_INFO).  A bad input leaves its bits in counts[1] and every other
    output zero."""
    return _global_positions(_Host, "global_positions_host", "global_positions",
                             (offsets, obs_image, obs_xy, cam_offsets, cam_obs, K, R, in_graph, tree_image, tree_t), root, huber, max_iters,
                             pcg_iters, pcg_tol, ftol, min_cam_obs, None)


@_on_device
def global_positions(offsets, obs_image, obs_xy, cam_offsets, cam_obs, K, R, in_graph, tree_image, tree_t, root, huber=0.1, max_iters=50,
                     pcg_iters=30, pcg_tol=1e-2, ftol=1e-7, min_cam_obs=8, timings=None):
    """loftr_global_positions: the kernels (csrc/position_gpu.hip) on GPU tensors of the dtypes and shapes of global_positions_host; the
    same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are in counts[1], which the caller
    reads once (every other output is then zero).  timings: a list that receives (stage, ms) pairs (the call then waits for the
    stream)."""
    return _global_positions(_Gpu, "global_positions",
                             "the global-positioning kernels have no CPU fallback; the host routine is global_positions_host",
                             (offsets, obs_image, obs_xy, cam_offsets, cam_obs, K, R, in_graph, tree_image, tree_t), root, huber, max_iters,
                             pcg_iters, pcg_tol, ftol, min_cam_obs, timings)
