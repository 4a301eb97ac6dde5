"""oracle/philox.py - the CPU restatement of the engine's device-noise generator - pinned on its own, without a GPU:
the published Philox4x32-10 known answers, the prefix property the engine's noise sharing rests on, the separation of the
engine's streams and steps in the counter, and the statistics of the normals.  tests/test_device_noise_gpu.py then holds the
HIP kernel to this restatement element by element and replays it into the CPU oracle."""
import numpy as np
import pytest

from oracle import philox as P

# the stream ids the engine passes to philox_normal / philox_normal_streams, restated (not imported) with their call sites
ENGINE_STREAMS = {
    "start": 0,                               # engine.hip:2178 (q_sample start), :2175 (seeded); model.py:538 / :773 (white start)
    "edm_start": 1,                           # model.py:967 / :971 (canvas_noise(1))
    "tiles": 1 << 32,                         # engine.hip:2011, :2009 (seeded): per-step tile noise, step mixed in
    "ring": (1 << 32) | 0x80000000,           # engine.hip:2062, :2059 (seeded), :1864 (EDM): ring re-noise, step mixed in
    "edm_eps": 2 << 32,                       # engine.hip:1820: EDM eps canvas, step mixed in
}


def test_stream_constants_of_the_restatement_are_the_engines():
    assert (P.STREAM_START, P.STREAM_EDM_START, P.STREAM_TILES, P.STREAM_RING, P.STREAM_EDM_EPS) == \
        tuple(ENGINE_STREAMS[k] for k in ("start", "edm_start", "tiles", "ring", "edm_eps"))


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox4x32_10_known_answers(counter, key, want):
    # the three vectors published with Random123 (kat_vectors, philox4x32 10 rounds)
    got = P.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join("%08x" % v for v in got) == want


def test_philox4x32_10_is_vectorised_over_quads():
    q = np.arange(7, dtype=np.uint64)
    both = P.philox4x32_10((q, 0, 3, 9), (71, 2))
    assert both.shape == (7, 4)
    for i in range(7):
        assert np.array_equal(both[i], P.philox4x32_10((i, 0, 3, 9), (71, 2)))
    assert len({tuple(r) for r in both}) == 7


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023])
def test_prefix_property(n, dtype):
    # a shorter draw is a prefix of a longer one of the same (seed, stream, step): a smaller image of a mixed-size group reads
    # the head of the largest image's tile noise
    for k in (1, 2, 3, 4, 1025):
        a = P.philox_normal(n, 71, P.STREAM_TILES, 3, dtype=dtype)
        b = P.philox_normal(n + k, 71, P.STREAM_TILES, 3, dtype=dtype)
        assert a.shape == (n,) and a.dtype == dtype
        assert np.array_equal(a, b[:n]), (n, k)


def test_output_order_and_tail():
    w = P.philox_words(8, 5, 1, None)
    z = P.box_muller(w)
    u1 = (w[:, 0].astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -32)
    th = np.float32(6.2831855) * (w[:, 1].astype(np.float32) * np.float32(2.0 ** -32))
    r = np.sqrt(-2 * np.log(u1.astype(np.float64)))
    assert np.array_equal(z[:, 0], r * np.cos(th.astype(np.float64))) and np.array_equal(z[:, 1], r * np.sin(th.astype(np.float64)))
    assert np.array_equal(P.philox_normal(7, 5, 1), z.reshape(-1)[:7])
    assert P.philox_normal(0, 5, 1).shape == (0,)


def test_streams_and_steps_are_separate_counters():
    # (c[2], c[3]) over every stream id of the engine x steps 0..1023 x {no step}: a collision would hand two different draws
    # the same normals.  "no step" (a null step_ptr) reads as step 0 in the kernel, so it coincides with step 0 of the SAME
    # stream - and with nothing else; the engine never draws one stream both ways (start streams: never a step; the others: always).
    words = {}
    for name, sid in ENGINE_STREAMS.items():
        for step in [None] + list(range(1024)):
            words.setdefault(P.counter_words(sid, step), []).append((name, step))
    for w, users in words.items():
        assert 0 <= w[0] <= 0xFFFFFFFF and 0 <= w[1] <= 0xFFFFFFFF
        if len(users) > 1:
            assert sorted(users, key=str) == sorted([(users[0][0], None), (users[0][0], 0)], key=str), users
    assert len(words) == len(ENGINE_STREAMS) * 1024
    for name, sid in ENGINE_STREAMS.items():
        assert P.counter_words(sid, None) == P.counter_words(sid, 0)
    # and the normals differ accordingly
    a = P.philox_normal(64, 71, P.STREAM_TILES, 1)
    assert not np.array_equal(a, P.philox_normal(64, 71, P.STREAM_TILES, 2))
    assert not np.array_equal(a, P.philox_normal(64, 71, P.STREAM_RING, 1))
    assert not np.array_equal(a, P.philox_normal(64, 72, P.STREAM_TILES, 1))
    assert np.array_equal(P.philox_normal(64, 71, P.STREAM_START, None), P.philox_normal(64, 71, P.STREAM_START, 0))


def test_step_limit_is_24_bits():
    # step << 8 in a 32-bit word: steps 0 .. 2^24 - 1 are distinct, 2^24 wraps onto 0 (documented in DESIGN.md).  The stream ids
    # keep to bits 0..1 of the high word, so no step below 2^24 can turn one stream's word into another's either.
    sid = P.STREAM_TILES
    assert P.counter_words(sid, (1 << 24) - 1) != P.counter_words(sid, 0)
    assert P.counter_words(sid, 1 << 24) == P.counter_words(sid, 0)
    assert P.counter_words(sid, (1 << 24) + 5) == P.counter_words(sid, 5)
    assert all(((s >> 32) & 0xFFFFFFFF) < (1 << 8) for s in ENGINE_STREAMS.values())


def test_seed_is_the_key_in_both_halves():
    a = P.philox_normal(16, 7, 0)
    assert not np.array_equal(a, P.philox_normal(16, 7 + 2 ** 32, 0))        # high key word
    assert np.array_equal(a, P.philox_normal(16, 7 + 2 ** 64, 0))            # the ABI passes uint64


def test_normals_statistics_and_range():
    # 3 * 768^2 normals (one ring canvas): N(0,1) moments within ~5 standard errors (se: mean 7.5e-4, std 5.3e-4, skew 2.9e-3,
    # 4th moment 7.4e-3), and the hard range of this Box-Muller: u1 >= 2^-32 bounds the radius by sqrt(64 ln 2) = 6.6604
    n = 3 * 768 * 768
    z = P.philox_normal(n, 71, P.STREAM_RING, 1)
    assert z.dtype == np.float64 and np.isfinite(z).all()
    assert abs(z.mean()) < 4e-3 and abs(z.std() - 1) < 3e-3
    assert abs((z ** 3).mean()) < 1.5e-2 and abs((z ** 4).mean() - 3.0) < 4e-2
    assert np.abs(z).max() <= np.sqrt(64 * np.log(2.0)) + 1e-12
    z2 = P.philox_normal(n, 71, P.STREAM_TILES, 1)
    assert abs((z * z2).mean()) < 4e-3                                        # two streams: uncorrelated
    assert abs((z[:-1] * z[1:]).mean()) < 4e-3                                # neighbours (cos / sin of one pair, and across pairs)
    # this very buffer holds u1 == 1.0 (a word >= 2^32 - 128 rounds to 2^32 in float32): radius 0, a zero, not a NaN
    w = P.philox_words(n, 71, P.STREAM_RING, 1)
    assert (w[:, [0, 2]] >= 0xFFFFFF80).any()
    z32 = P.philox_normal(n, 71, P.STREAM_RING, 1, dtype=np.float32)
    assert z32.dtype == np.float32 and np.isfinite(z32).all()
    # the float32 twin sits at float32 rounding distance from the float64 value (a few ulps at |z| <= 6.66)
    assert np.abs(z32.astype(np.float64) - z).max() < 2e-6


def test_box_muller_edges_give_no_nan():
    top = np.array([[0xFFFFFFFF] * 4, [0xFFFFFF80, 0, 0, 0xFFFFFFFF], [0, 0, 0, 0]], dtype=np.uint32)
    for dtype in (np.float64, np.float32):
        z = P.box_muller(top, dtype)
        assert np.isfinite(z).all()
        assert np.all(z[0] == 0) and z[1, 0] == 0 and z[1, 1] == 0            # u1 = 1: radius 0
        assert abs(z[2, 0] - np.sqrt(64 * np.log(2.0))) < 1e-5 and z[2, 1] == 0    # u1 = 2^-32, theta = 0: the largest value


def test_draw_plans_have_the_oracles_shapes_and_order():
    # the plan is consumed by srgd_oracle.ReplayNoise, which asserts every shape; here: counts, order and provenance
    n = 3 * 256 * 256
    d = P.device_noise_draws("ddpm_tiled", seed=71, num_sample_steps=4, height=136, width=200, batch_size=4)
    assert [tuple(t.shape) for t in d] == [(1, 3, 256, 256), (1, 3, 256, 256), (1, 3, 256, 256), (1, 3, 256, 256),
                                           (1, 3, 256, 256), (1, 3, 256, 256)]   # start, t0, t1, ring1, t2, ring3
    want = [(0, None), (1 << 32, 0), (1 << 32, 1), ((1 << 32) | 0x80000000, 1), (1 << 32, 2), ((1 << 32) | 0x80000000, 3)]
    for t, (sid, step) in zip(d, want):
        assert np.array_equal(t.reshape(-1).numpy(), P.philox_normal(n, 71, sid, step).astype(np.float32))
    # a skipped prefix keeps the loop index as the step value
    d = P.device_noise_draws("ddpm_tiled", seed=71, num_sample_steps=4, generation_start_steps=2, height=136, width=200)
    assert len(d) == 3
    assert np.array_equal(d[1].reshape(-1).numpy(), P.philox_normal(n, 71, 1 << 32, 2).astype(np.float32))
    # 768^2 canvas, 9 tiles in minibatches of 4: slices of ONE buffer
    d = P.device_noise_draws("ddpm_tiled", seed=3, num_sample_steps=2, height=264, width=272, batch_size=4)
    assert [tuple(t.shape) for t in d] == [(1, 3, 768, 768), (4, 3, 256, 256), (4, 3, 256, 256), (1, 3, 256, 256), (1, 3, 768, 768)]
    buf = P.philox_normal(9 * n, 3, 1 << 32, 0).astype(np.float32)
    assert np.array_equal(np.concatenate([t.reshape(-1).numpy() for t in d[1:4]]), buf)
    d = P.device_noise_draws("edm_tiled", seed=3, num_sample_steps=3, height=136, width=200)
    assert len(d) == 1 + 3 + 1
    assert np.array_equal(d[0].reshape(-1).numpy(), P.philox_normal(n, 3, 1).astype(np.float32))
    assert np.array_equal(d[2].reshape(-1).numpy(), P.philox_normal(n, 3, 2 << 32, 1).astype(np.float32))
    d = P.device_noise_draws("ddpm_sample", seed=3, num_sample_steps=3, batch=2)
    assert [tuple(t.shape) for t in d] == [(2, 3, 256, 256)] * 3
    start = P.philox_normal(2 * n, 3, 0).astype(np.float32).reshape(3, 2 * 256, 256)       # canvas layout [3][b*S][S]
    assert np.array_equal(d[0][1, 2].numpy(), start[2, 256:512])
