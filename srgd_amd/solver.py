"""Few-step samplers of the tiled DDPM loop (engine extension, absent upstream): the step tables of DDIM and of the second-order
multistep solver DPM-Solver++ 2M in float64, and the solver's history step on the GPU - ``srgd_solver_history_step`` of
``libsrgd_solver.so`` (srgd_amd/csrc/solver.hip, the definition is fixed in include/srgd_solver.h; a library of its own beside the
engine's, the metrics', the ensemble's, the consistency's, the back-projection's and the guidance's, built by the same
srgd_amd/build.py).  The engine's step kernel computes ``alpha_next * (x_t * one_minus_c / alpha + c * x0) + noise_scale * z`` from a
host table, so any update ``A x_t + B x0 + S z`` is a table; the 2M step adds ``w (x0 - x0_prev)`` inside every image's inner box.
There is no CPU path and no torch arithmetic on the canvases here: the caller owns every buffer."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib

SAMPLERS = ("ddpm", "ddim", "dpmpp2m")
SPACINGS = ("time", "logsnr")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_solver.so")


class SolverImage(C.Structure):
    """``srgd_solver_image`` of include/srgd_solver.h."""
    _fields_ = [("canvas_off", C.c_int64), ("Hp", C.c_int32), ("Wp", C.c_int32), ("top", C.c_int32), ("left", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32)]


# name -> (restype, argtypes); every symbol include/srgd_solver.h declares
PROTOTYPES = {
    "srgd_solver_last_error": (C.c_char_p, []),
    "srgd_solver_history_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SolverImage), C.c_int, C.c_float, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the solver library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The solver's history step runs on the MI355X only")
    return _handle


def check_sampler(sampler="ddpm", eta=None, step_spacing="time"):
    """``tiled_sample(sampler=, eta=, step_spacing=)`` -> ``(sampler, eta, step_spacing)`` with ``eta`` None for "ddpm" and a float
    for the other two (0.0 when not given); anything else raises ``ValueError``."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler: one of {', '.join(SAMPLERS)}, got {sampler!r}")
    if step_spacing not in SPACINGS:
        raise ValueError(f"step_spacing: one of {', '.join(SPACINGS)}, got {step_spacing!r}")
    if eta is not None and (isinstance(eta, bool) or not isinstance(eta, (int, float)) or not math.isfinite(eta)
                            or not 0.0 <= eta <= 1.0):
        raise ValueError(f"eta: a number in [0, 1], got {eta!r}")
    if sampler == "ddpm":
        if eta is not None:
            raise ValueError(f"eta: the ddpm sampler takes none (its step is the ancestral one), got {eta!r}")
        return sampler, None, step_spacing
    if sampler == "dpmpp2m" and eta:
        raise ValueError(f"eta: the dpmpp2m sampler is deterministic (None or 0), got {eta!r}")
    return sampler, float(eta or 0.0), step_spacing


def is_default(sampler, eta, step_spacing):
    return sampler == "ddpm" and eta is None and step_spacing == "time"


def step_coefficients(log_snr, log_snr_next, eta):
    """(A, B, S) of the update ``A x_t + B x0 + S z`` from the log-SNR at the step's start and end, in float64 (Python floats):
    c0 = -expm1(l - l'), s~^2 = s'^2 c0, k = sqrt(s'^2 - eta^2 s~^2), A = k / s, B = a' - k a / s, S = eta s~ - the DDIM family; eta = 1
    is the ancestral DDPM step."""
    l0, l1, eta = float(log_snr), float(log_snr_next), float(eta)
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))              # noqa: E731
    alpha, sigma = math.sqrt(sig(l0)), math.sqrt(sig(-l0))
    alpha_next, var_next = math.sqrt(sig(l1)), sig(-l1)
    c0 = -math.expm1(l0 - l1)
    var = var_next * c0
    k = math.sqrt(var_next - eta * eta * var)
    return k / sigma, alpha_next - k * alpha / sigma, eta * math.sqrt(var)


def history_weights(levels, first_step=0):
    """The 2M history weights of a run over the N + 1 log-SNR ``levels``: w_i = B_i / (2 r_i) with B_i of eta = 0,
    r_i = h_{i-1} / h_i, h_i = (l'_i - l_i) / 2; 0 on the first executed step (there is no history yet), on the last one (lower-order
    final step) and on the steps that are skipped."""
    lv = [float(v) for v in levels]
    n = len(lv) - 1
    out = [0.0] * n
    for i in range(max(first_step, 0) + 1, n - 1):
        r = (lv[i] - lv[i - 1]) / (lv[i + 1] - lv[i])
        out[i] = step_coefficients(lv[i], lv[i + 1], 0.0)[1] / (2.0 * r)
    return out


def records(images):
    """The host record array of a run: ``images`` = ``[(canvas_off, Hp, Wp, top, left, h, w)]`` with the inner box of every image.
    ``ValueError`` for a box that leaves its canvas."""
    if not images:
        raise ValueError("solver: no images")
    recs = (SolverImage * len(images))()
    for r, m in zip(recs, images):
        canvas_off, hp, wp, top, left, h, w = (int(v) for v in m)
        if canvas_off < 0 or top < 0 or left < 0 or h < 1 or w < 1 or top + h > hp or left + w > wp or 3 * hp * wp >= 2 ** 31:
            raise ValueError(f"solver: bad canvas {hp}x{wp} / box {h}x{w} at ({top}, {left}) / offset {canvas_off}")
        r.canvas_off, r.Hp, r.Wp, r.top, r.left, r.h, r.w = canvas_off, hp, wp, top, left, h, w
    return recs


def history_step_flat(img, x_start, x_prev, recs, w):
    """One batched call on flat fp32 device buffers, in place on ``img`` and ``x_prev``: ``recs`` from ``records`` (image i's
    ``[3,Hp,Wp]`` canvas starts at ``canvas_off`` of all three).  No allocation, no synchronisation."""
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w):
        raise ValueError(f"solver: the weight must be a finite number, got {w!r}")
    if not isinstance(recs, C.Array) or recs._type_ is not SolverImage or len(recs) < 1:
        raise ValueError("solver: recs is the record array records() returns")
    for t in (img, x_start, x_prev):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("solver: contiguous fp32 buffers")
    if max(r.canvas_off + 3 * r.Hp * r.Wp for r in recs) > min(img.numel(), x_start.numel(), x_prev.numel()):
        raise ValueError("solver: records do not fit the buffers")
    if len({img.device, x_start.device, x_prev.device}) != 1:
        raise ValueError("solver: buffers on one device")
    if not img.is_cuda:
        raise _lib.SrgdHipError("the solver's history step runs on MI355X only (no CPU fallback)")
    with torch.cuda.device(img.device):
        rc = lib().srgd_solver_history_step(C.c_void_p(img.data_ptr()), C.c_void_p(x_start.data_ptr()), C.c_void_p(x_prev.data_ptr()),
                                            recs, len(recs), float(w), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_solver_last_error")
