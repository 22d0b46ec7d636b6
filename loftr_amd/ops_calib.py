"""Python wrappers of libloftr_calib.so (include/loftr_calib.h): view-graph calibration (csrc/calib.hip, csrc/calib_gpu.hip; DESIGN
§28).  The two sides of the routine share one body, written against the backends of ``ops`` (``_Host`` on numpy arrays defines the
result, ``_Gpu`` on GPU tensors reproduces it); the third library is loaded lazily, on the first call."""
import math

from . import _lib
from .ops import _Gpu, _Host, _StageMs, _check_args, _on_device, _outputs, _stream

CALIB_COUNTS = 16
CALIB_NAMES = ("n_trials", "error_bits", "n_accepted", "n_pcg_iters", "n_valid_edges", "n_free_groups", "n_outlier_edges", "status",
               "n_bound_rejections")                                                       # counts[0..8]
CALIB_INFO = ("cost_start", "cost_end", "lambda", "last_step")                            # info[0..3]
CALIB_STATUS = ("converged", "max_iters", "stalled", "nothing")                           # counts[7]
CALIB_EDGE_STATES = ("invalid", "ok", "outlier")                                          # edge_state codes 0..2
CALIB_GROUP_STATES = ("no_valid_edge", "held", "refined")                                 # group_state codes 0..2
CALIB_STAGES = ("check", "setup", "refine", "write")
CALIB_ERRORS = ((1, "an edge image outside [0, n_images), or an edge from an image to itself"),
                (2, "a group outside [0, n_groups)"),
                (4, "grp_offsets / grp_inc must group the edge ends by camera in ascending order"),
                (8, "f0 must be finite and positive and principal_point finite"))          # bits of counts[1]
CALIB_DEFAULTS = dict(loss=0.05, max_resid=0.05, prior_weight=1e-3, weight_cap=100, bound_lo=0.2, bound_hi=5.0, min_edges=1, max_iters=50,
                      pcg_iters=30, pcg_tol=1e-2, ftol=1e-9)
_CALIB_ARGS = (("edge_image", "int32", 2), ("edge_F", "float64", 3), ("edge_weight", "int32", 1), ("pp", "float64", 2), ("f0", "float64", 1),
               ("group", "int32", 1), ("grp_offsets", "int64", 1), ("grp_inc", "int32", 1))
_CALIB_OUT = (("focal_scale", "G", (), "float64"), ("focal", "n", (), "float64"), ("edge_resid", "E", (), "float64"),
              ("edge_state", "E", (), "uint8"), ("group_state", "G", (), "uint8"))


def check_params(what, loss, max_resid, prior_weight, weight_cap, bound_lo, bound_hi, min_edges, max_iters, pcg_iters, pcg_tol, ftol):
    """The ranges the C entry points answer with LOFTR_ERR_BAD_ARG, as ValueErrors that name the parameter."""
    for name, v, lo in (("weight_cap", weight_cap, 1), ("min_edges", min_edges, 0), ("max_iters", max_iters, 0), ("pcg_iters", pcg_iters, 0)):
        if not isinstance(v, int) or isinstance(v, bool) or v < lo:
            raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")
    if max_iters > 1 << 16 or pcg_iters > 1 << 16:
        raise ValueError(f"{what}: max_iters and pcg_iters must be at most {1 << 16}")
    fl = dict(loss=loss, max_resid=max_resid, prior_weight=prior_weight, bound_lo=bound_lo, bound_hi=bound_hi, pcg_tol=pcg_tol, ftol=ftol)
    for name, v in fl.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    if not loss > 0 or max_resid < 0 or prior_weight < 0 or ftol < 0:
        raise ValueError(f"{what}: loss must be > 0 and max_resid, prior_weight and ftol >= 0, got {loss!r}, {max_resid!r}, "
                         f"{prior_weight!r}, {ftol!r}")
    if not 0 < bound_lo < 1 < bound_hi:
        raise ValueError(f"{what}: the bounds must satisfy 0 < bound_lo < 1 < bound_hi, got ({bound_lo!r}, {bound_hi!r})")
    if not 0 <= pcg_tol < 1:
        raise ValueError(f"{what}: pcg_tol must lie in [0, 1), got {pcg_tol!r}")


def _calibrate(B, what, hint, arrays, params, timings):
    from . import _lib_calib
    _check_args(B, what, hint, _CALIB_ARGS, arrays)
    edge_image, edge_F, edge_weight, pp, f0, group, grp_offsets, grp_inc = arrays
    E, n, G = edge_image.shape[0], f0.shape[0], grp_offsets.shape[0] - 1
    p = {**CALIB_DEFAULTS, **params}
    if set(p) != set(CALIB_DEFAULTS):
        raise TypeError(f"{what}: unknown parameter(s) {sorted(set(p) - set(CALIB_DEFAULTS))}")
    check_params(what, **p)
    if (n < 1 or G < 1 or G > n or tuple(edge_image.shape) != (E, 2) or tuple(edge_F.shape) != (E, 3, 3) or edge_weight.shape[0] != E
            or tuple(pp.shape) != (n, 2) or group.shape[0] != n or grp_inc.shape[0] != 2 * E):
        raise _lib.LoftrHipError(f"{what}: expected edge_image [E,2], edge_F [E,3,3], edge_weight [E], pp [n,2], f0 [n], group [n] with "
                                 f"n >= 1, grp_offsets [G+1] with 1 <= G <= n and grp_inc [2E], got {[tuple(a.shape) for a in arrays]}")
    arrays = [B.contiguous(x) for x in arrays]                                           # (held until the call has returned)
    a = [B.ptr(x) for x in arrays]
    out = _outputs(B, _CALIB_OUT, {"G": G, "n": n, "E": E}, CALIB_COUNTS, f0)
    out["info"] = B.zeros(len(CALIB_INFO), "float64", f0)
    args = (a[0], a[1], a[2], E, a[3], a[4], a[5], n, G, a[6], a[7], float(p["loss"]), float(p["max_resid"]), float(p["prior_weight"]),
            p["weight_cap"], float(p["bound_lo"]), float(p["bound_hi"]), p["min_edges"], p["max_iters"], p["pcg_iters"], float(p["pcg_tol"]),
            float(p["ftol"]), *[B.ptr(out[k]) for k in out])
    lib = _lib_calib.load()
    if B is _Host:
        status = lib.loftr_calibrate_view_graph_host(*args)
        if not (status == -1 and int(out["counts"][1]) != 0):                            # a bad input is reported through counts[1], as on the GPU
            _lib_calib.check(status, "loftr_calibrate_view_graph_host")
        return out
    import torch
    ms = _StageMs(timings, CALIB_STAGES)
    buf = torch.empty(max(1, lib.loftr_calibrate_view_graph_workspace_bytes(E, n, G)), dtype=torch.uint8, device=f0.device)
    _lib_calib.check(lib.loftr_calibrate_view_graph(*args, B.ptr(buf), buf.numel(), ms.arg, _stream()), "loftr_calibrate_view_graph")
    ms.report()
    return out


def calibrate_view_graph_host(edge_image, edge_F, edge_weight, pp, f0, group, grp_offsets, grp_inc, **params):
    """loftr_calibrate_view_graph_host: the host routine that DEFINES view-graph calibration (include/loftr_calib.h) on
    numpy arrays: edge_image [E,2] i32, edge_F [E,3,3] f64, edge_weight [E] i32, pp [n,2] f64, f0 [n] f64, group [n] i32, grp_offsets
    [G+1] i64, grp_inc [2E] i32.  params: CALIB_DEFAULTS (a prototype's values, UNVALIDATED on real data).
    -> dict of numpy arrays: focal_scale [G] f64, focal [n] f64, edge_resid [E] f64, edge_state [E] u8, group_state [G] u8, counts [16]
    i64 (CALIB_NAMES), info [4] f64 (CALIB_INFO).  A bad input leaves its bits in counts[1] and every other output zero."""
    return _calibrate(_Host, "calibrate_view_graph_host", "calibrate_view_graph",
                      (edge_image, edge_F, edge_weight, pp, f0, group, grp_offsets, grp_inc), params, None)


@_on_device
def calibrate_view_graph(edge_image, edge_F, edge_weight, pp, f0, group, grp_offsets, grp_inc, timings=None, **params):
    """loftr_calibrate_view_graph: the kernels (csrc/calib_gpu.hip) on GPU tensors of the dtypes and shapes of
    calibrate_view_graph_host; the same result bit for bit.  -> dict of device tensors; nothing is read back here: the error bits are
    in counts[1], which the caller reads once (every other output is then zero).  timings: a list that receives (stage, ms) pairs (the
    call then waits for the stream)."""
    return _calibrate(_Gpu, "calibrate_view_graph",
                      "the calibration kernels have no CPU fallback; the host routine is calibrate_view_graph_host",
                      (edge_image, edge_F, edge_weight, pp, f0, group, grp_offsets, grp_inc), params, timings)
