"""HIP-event timing of the ensemble kernels (srgd_image_ensemble_images) against the same definition written in torch on the same GPU
(int64 sums, the rounded mean, the spread as floor(2 sqrt(D) / K + 0.5) in float64, mean01, the two statistics):

    python tools/bench_ensemble.py [--out profiles/ensemble_bench.txt] [--note "box / commit"]

Cases: K = 5 samples of a group of 20 BSD100-shaped x4 outputs (1920x1280) in one batched call, and of one 8192^2 output, each with
and without mean01.  Every figure is the median over --repeats samples, each sample `inner` back-to-back calls between two HIP events,
after --warmup untimed calls of the same shape; outputs and scratch are allocated outside the timed window, and the copy of the
statistics to the host is not timed.  The rate is (K + 2) * 3hw bytes (+ 12 hw with mean01) over the kernels' time.  The file also
records the kernels' registers, LDS bytes and scratch from the compiler's resource table (tools/kernel_resources.py) and whether
the two sides agree.  Nothing is gated.  Needs the MI355X; there is no CPU path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import ensemble as EN                         # noqa: E402


def timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / inner)
    return statistics.median(samples), min(samples), max(samples)


def torch_ensemble(x, with_mean01):
    """The definition in torch on the device: uint8 [K,h,w,3] -> (mean uint8, spread uint8, mean01 or None, [2] float64).  The spread
    is taken in float64 (floor(2 sqrt(D) / K + 0.5)), which the CPU suite shows to equal the integer rule on random data."""
    k = x.shape[0]
    v = x.to(torch.int64)
    s, q = v.sum(0), (v * v).sum(0)
    d = k * q - s * s
    mean = ((2 * s + k) // (2 * k)).to(torch.uint8)
    root = d.double().sqrt()
    spread = torch.floor(2.0 * root / k + 0.5).to(torch.uint8)
    m01 = (mean.float() / 255.0).permute(2, 0, 1).contiguous() if with_mean01 else None
    return mean, spread, m01, torch.stack([(root.sum() / k) / d.numel(), d.max().double().sqrt() / k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip_8192", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs the MI355X: no GPU visible and there is no CPU path")
    L = EN.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    k = args.samples
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# ensemble (mean image, spread map, mean01, mean_std / max_std) of K = {k} samples: HIP kernels against the same definition in "
         "torch (same GPU), HIP events, median [min, max] ms per call")
    emit(f"# command: python tools/bench_ensemble.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls per shape, {args.repeats} samples; sample = `inner` back-to-back calls between two events")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "ensemble.hip")):
            if "ensemble_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    cases = [("20 x 1280x1920 (one batched call)", 20, 1280, 1920, 5)] + ([] if args.skip_8192 else [("1 x 8192x8192", 1, 8192, 8192, 2)])
    for name, n, h, w, inner in cases:
        e = 3 * h * w                                        # a multiple of 16 for both shapes: no padding
        assert e % EN.VEC == 0
        x = torch.randint(0, 256, (n * k * e,), generator=g, device="cuda", dtype=torch.uint8)
        s_offs = (C.c_int64 * n)(*[i * k * e for i in range(n)])
        o_offs = (C.c_int64 * n)(*[i * e for i in range(n)])
        hw = (C.c_int32 * (2 * n))(*([h, w] * n))
        mean = torch.empty(n * e, device="cuda", dtype=torch.uint8)
        spread = torch.empty(n * e, device="cuda", dtype=torch.uint8)
        m01 = torch.empty(n * e, device="cuda", dtype=torch.float32)
        stats = torch.empty(n, 2, device="cuda", dtype=torch.float64)
        scratch = torch.empty(EN.scratch_doubles([(h, w)] * n), device="cuda", dtype=torch.float64)
        for with_m01 in (False, True):
            def kernels():
                rc = L.srgd_image_ensemble_images(p(x), s_offs, hw, n, k, p(mean), p(spread), o_offs, p(m01) if with_m01 else None,
                                                  o_offs if with_m01 else None, p(stats), p(scratch), st)
                assert rc == 0, L.srgd_image_ensemble_last_error()

            def restatement():
                return [torch_ensemble(x[i * k * e:(i + 1) * k * e].view(k, h, w, 3), with_m01) for i in range(n)]
            tk = timed(kernels, args.warmup, args.repeats, inner)
            tt = timed(restatement, 1, max(3, args.repeats // 2), 1)
            nbytes = n * ((k + 2) * e + (4 * e if with_m01 else 0))
            agree = True
            for i, (t_mean, t_spread, t_m01, t_stats) in enumerate(restatement()):
                agree &= torch.equal(t_mean.reshape(-1), mean[i * e:(i + 1) * e]) and torch.equal(t_spread.reshape(-1), spread[i * e:(i + 1) * e])
                agree &= (not with_m01) or torch.equal(t_m01.reshape(-1), m01[i * e:(i + 1) * e])
                agree &= bool((t_stats - stats[i]).abs().max() <= 1e-9)
            emit(f"{name}, {'with' if with_m01 else 'without'} mean01: kernels {tk[0]:.3f} [{tk[1]:.3f}, {tk[2]:.3f}] ms = "
                 f"{nbytes / tk[0] / 1e9:.2f} TB/s of {nbytes / 1e6:.0f} MB; torch {tt[0]:.3f} [{tt[1]:.3f}, {tt[2]:.3f}] ms; "
                 f"ratio x{tt[0] / tk[0]:.1f}; outputs {'agree' if agree else 'DISAGREE'}")
        s0 = stats[0].cpu().tolist()
        emit(f"  image 0: mean_std {s0[0]:.9f}, max_std {s0[1]:.9f} (8-bit units)")
        del x, mean, spread, m01, stats, scratch
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
