"""Time of what ``--self_ensemble 8`` adds after sampling (``srgd_amd.selfens``) on the MI355X against the same composition in torch ops
on the same GPU and in numpy on the CPU:

    python tools/time_selfens.py [--out profiles/selfens_bench.txt] [--note "box / commit"] [--append]

Merge: ``--images`` (5) outputs of ``--size`` x ``--size`` (2048) pixels, each from N = ``--n`` (8) sources - the outputs of the
orientations of ``OPS[N]``, resident on the GPU in one flat buffer.  After ``--warmup`` untimed calls, the median of ``--repeats``
``merge_flat`` calls (one launch), each between two HIP events; the bytes per second - ``(N + 1) * 3 * H * W`` bytes per image: every
source byte read once, every output byte written once - are printed beside the HBM figure of the box (``--hbm_tbs``, 8 TB/s by
specification).  The same with ``mean01`` (12 more bytes written per pixel), the list API ``self_ensemble_on_device`` (which also
packs the sources into its flat buffer) and the forward transform of the five inputs' eight orientations.  Beside them the same
composition in torch ops (``flip`` / ``transpose`` / sum in int32 / halves-up division) on the same GPU, and the numpy restatement
on this machine's CPU.  Every GPU result is compared with the numpy restatement, byte for byte, before anything is timed.  Nothing
is gated.  Needs the MI355X."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srgd_amd import selfens as SE                          # noqa: E402
from tests import selfens_cases as SC                       # noqa: E402


def torch_turn_back(t, op):
    """``apply(t, inverse(op))`` in torch ops."""
    op = SE.inverse(op)
    t = t.transpose(0, 1) if op & 4 else t
    t = t.flip(1) if op & 1 else t
    return t.flip(0) if op & 2 else t


def torch_merge(sources, ops):
    total = sum(torch_turn_back(s, op).to(torch.int32) for s, op in zip(sources, ops))
    n = len(ops)
    return torch.div(2 * total + n, 2 * n, rounding_mode="floor").to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfens_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--n", type=int, default=8, choices=[2, 4, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--hbm_tbs", type=float, default=8.0, help="the box's HBM bandwidth in TB/s, printed beside the merge's rate")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_selfens needs the MI355X: no GPU visible and there is no CPU path")
    device = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        samples = []
        for k in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if k >= args.warmup:
                samples.append(a.elapsed_time(b))
        return statistics.median(samples), min(samples), max(samples)

    n_img, size, n = args.images, args.size, args.n
    ops = list(SE.OPS[n])
    emit(f"# self-ensemble (srgd_amd.selfens): {n_img} x {size}x{size} RGB outputs, N = {n} sources each; HIP events, median [min, max] ms "
         "per call")
    emit(f"# command: python tools/time_selfens.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls, {args.repeats} samples")
    rng = np.random.default_rng(0)
    sources = [[SC.apply(rng.integers(0, 256, (size, size, 3), dtype=np.uint8), op) for op in ops] for _ in range(n_img)]
    t0 = time.perf_counter()
    want = [SC.merge(s, ops) for s in sources]
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    nbytes = 3 * size * size
    src = torch.cat([torch.from_numpy(s.reshape(-1)) for group in sources for s in group]).to(device)
    src_offsets = [[(i * n + j) * nbytes for j in range(n)] for i in range(n_img)]
    dst_offsets = [i * nbytes for i in range(n_img)]
    dst = torch.empty(n_img * nbytes, device=device, dtype=torch.uint8)
    m01 = torch.empty(n_img * nbytes, device=device, dtype=torch.float32)
    sizes = [(size, size)] * n_img
    SE.merge_flat(src, src_offsets, [ops] * n_img, dst, dst_offsets, sizes, m01, dst_offsets)
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        assert np.array_equal(dst[i * nbytes:(i + 1) * nbytes].view(size, size, 3).cpu().numpy(), w)
        assert np.array_equal(m01[i * nbytes:(i + 1) * nbytes].view(3, size, size).cpu().numpy().view(np.uint32), SC.mean01(w).view(np.uint32))
    moved = (n + 1) * nbytes * n_img
    m, lo, hi = timed(lambda: SE.merge_flat(src, src_offsets, [ops] * n_img, dst, dst_offsets, sizes))
    emit(f"merge, {n_img} x {size}x{size}, N = {n}, on resident flat buffers, one launch: {m:.3f} [{lo:.3f}, {hi:.3f}] ms per call, "
         f"{moved / 1e6:.0f} MB by definition ((N + 1) * 3 * H * W per image) = {moved / m / 1e9:.2f} TB/s; HBM of the box: {args.hbm_tbs:g} "
         f"TB/s ({100 * moved / m / 1e9 / args.hbm_tbs:.0f} %); equal to the numpy restatement byte for byte")
    m2, lo, hi = timed(lambda: SE.merge_flat(src, src_offsets, [ops] * n_img, dst, dst_offsets, sizes, m01, dst_offsets))
    moved2 = moved + 4 * nbytes * n_img
    emit(f"merge with mean01 (fp32 planes, 12 more bytes written per pixel): {m2:.3f} [{lo:.3f}, {hi:.3f}] ms per call, "
         f"{moved2 / 1e6:.0f} MB = {moved2 / m2 / 1e9:.2f} TB/s")
    groups = [[(src[o:o + nbytes].view(size, size, 3), op) for o, op in zip(offs, ops)] for offs in src_offsets]
    got = SE.self_ensemble_on_device(groups)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    m3, lo, hi = timed(lambda: SE.self_ensemble_on_device(groups))
    emit(f"self_ensemble_on_device (the list API: allocates, copies the {n * n_img} sources into its flat buffer, one launch): {m3:.3f} "
         f"[{lo:.3f}, {hi:.3f}] ms per call")
    got = [torch_merge([t for t, _ in g], ops) for g in groups]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    m4, lo, hi = timed(lambda: [torch_merge([t for t, _ in g], ops) for g in groups])
    emit(f"the same composition in torch ops on the same GPU (flip / transpose / int32 sum / floor division): {m4:.3f} [{lo:.3f}, {hi:.3f}] ms "
         f"per call; torch / kernel = {m4 / m:.1f} x")
    emit(f"the numpy restatement (int64 sums) on this machine's CPU: {numpy_ms:.0f} ms; numpy / kernel = {numpy_ms / m:.0f} x")
    del got, groups
    low = size // 4                                        # the forward side: the eight orientations of five inputs
    inputs = [rng.integers(0, 256, (low, low, 3), dtype=np.uint8) for _ in range(n_img)]
    d_inputs = [torch.from_numpy(x).to(device) for x in inputs]
    images, image_ops = [t for t in d_inputs for _ in ops], ops * n_img
    turned = SE.dihedral_on_device(images, image_ops)
    assert all(np.array_equal(t.cpu().numpy(), SC.apply(inputs[i // n], op)) for i, (t, op) in enumerate(zip(turned, image_ops)))
    m5, lo, hi = timed(lambda: SE.dihedral_on_device(images, image_ops))
    emit(f"dihedral_on_device, {n_img} x {low}x{low} inputs x {n} ops in one call (list API): {m5:.3f} [{lo:.3f}, {hi:.3f}] ms per call, equal "
         "to the numpy restatement byte for byte")
    big = src[:nbytes * n].clone()                          # the transform kernel alone at output size: eight ops of one 2048^2 image
    out = torch.empty(nbytes * n, device=device, dtype=torch.uint8)
    offs = [j * nbytes for j in range(n)]
    SE.transform_flat(big, [0] * n, out, offs, [(size, size)] * n, ops)
    ref = big[:nbytes].view(size, size, 3).cpu().numpy()
    assert all(np.array_equal(out[o:o + nbytes].cpu().numpy().reshape(SE.out_size(size, size, op) + (3,)), SC.apply(ref, op)) for o, op in zip(offs, ops))
    m6, lo, hi = timed(lambda: SE.transform_flat(big, [0] * n, out, offs, [(size, size)] * n, ops))
    emit(f"transform alone, one {size}x{size} image x {n} ops on resident flat buffers, one launch: {m6:.3f} [{lo:.3f}, {hi:.3f}] ms per call, "
         f"{2 * n * nbytes / 1e6:.0f} MB read + written = {2 * n * nbytes / m6 / 1e9:.2f} TB/s")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
