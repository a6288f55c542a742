"""CPU tests of what StreamSession.push decides on the host, through the pure steps it calls: check_stream_chunks (every
refusal, in both loudness modes), stream_push_rows (the rows of a push against window_plan, their order, the forgetting
factors against running_horizon_rows one window at a time), StreamRow against the plain tuple in the stitch layout, and
the sizes the constructor resolves without a device."""
import dataclasses
import random
import types

import numpy as np
import pytest

from svcc23_fastsvc_amd import decode as Dc
from svcc23_fastsvc_amd import synth as S

C, HOP, MAX_PUSH = 5, 4, 3
SIZES = ((4, 4), (8, 4), (5, 8))            # (core, context)


def _chunk(n, sig="lft", hop=HOP, channels=C):
    return {"ppg": np.zeros((n, channels), np.float32), "f0": np.zeros(n, np.float32), sig: np.zeros(n * hop, np.float32)}


def _check(chunks, end=(), loudness="given", open_ids=(3, 7, 8)):
    return Dc.check_stream_chunks(chunks, end, {i: 0 for i in open_ids}, C, HOP, MAX_PUSH, loudness)


@pytest.mark.parametrize("loudness,sig,other", (("given", "lft", "audio"), ("audio", "audio", "lft")))
def test_check_stream_chunks_refuses(loudness, sig, other):
    good = _chunk(2, sig)
    bad = (
        (({99: good}, ()), "stream 99 is not open"),
        (({7: good}, (99,)), "stream 99 is not open"),
        (({7: good}, (7, 7)), "listed twice in end"),
        (({7: [1, 2, 3]}, ()), f"stream 7: a chunk is a dict with ppg, f0 and {sig}"),
        (({7: None}, ()), f"stream 7: a chunk is a dict with ppg, f0 and {sig}"),
        (({7: {k: v for k, v in good.items() if k != "f0"}}, ()), f"stream 7: a chunk is a dict with ppg, f0 and {sig}"),
        (({7: {k: v for k, v in good.items() if k != sig}}, ()), f"stream 7: a chunk is a dict with ppg, f0 and {sig}"),
        (({7: dict(good, **{other: good[sig]})}, ()), f"loudness=\"{loudness}\": a chunk carries {sig}, not {other}"),
        (({7: _chunk(2, other)}, ()), f"stream 7: a chunk is a dict with ppg, f0 and {sig}"),
        (({7: dict(good, ppg=good["ppg"][:, :-1])}, ()), r"stream 7: ppg must be \(n, 5\), got \(2, 4\)"),
        (({7: dict(good, ppg=good["ppg"][0])}, ()), r"stream 7: ppg must be \(n, 5\), got \(5,\)"),
        (({7: _chunk(4, sig)}, ()), "stream 7: 4 frames in one push, max_push is 3"),
        (({7: dict(good, f0=np.zeros(3))}, ()), r"stream 7: f0 must be \(2,\) or \(2, 1\), got \(3,\)"),
        (({7: dict(good, f0=np.zeros((1, 2)))}, ()), r"stream 7: f0 must be \(2,\) or \(2, 1\), got \(1, 2\)"),
        (({7: dict(good, **{sig: good[sig][:-1]})}, ()), rf"stream 7: {sig} must be \(8,\) or \(8, 1\), got \(7,\)"),
        (({7: dict(good, **{sig: np.zeros((2, HOP))})}, ()), rf"stream 7: {sig} must be \(8,\) or \(8, 1\), got \(2, 4\)"),
        (({3: good, 7: dict(good, f0=np.zeros(1))}, (8,)), "stream 7: f0 must be"),        # (a good chunk in front of a bad one)
    )
    for (chunks, end), what in bad:
        with pytest.raises(ValueError, match=what):
            _check(chunks, end, loudness)


@pytest.mark.parametrize("loudness,sig", (("given", "lft"), ("audio", "audio")))
def test_check_stream_chunks_accepts(loudness, sig):
    flat, column, empty = _chunk(3, sig), _chunk(2, sig), _chunk(0, sig)
    column = dict(column, f0=column["f0"].reshape(2, 1), **{sig: column[sig].reshape(2 * HOP, 1)})
    parts, ids, end = _check({7: flat, 3: column, 8: empty}, (np.int64(3),), loudness)
    assert list(parts) == [7, 3, 8] and ids == [7, 3, 8] and end == [3] and type(end[0]) is int
    for sid, n in ((7, 3), (3, 2), (8, 0)):
        k, ppg, f0, sg = parts[sid]
        assert k == n and ppg.shape == (n, C) and f0.shape == (n,) and sg.shape == (n * HOP,)
    parts, ids, end = _check({7: flat}, (8, 3), loudness)                # (ids that are in end only, behind the chunks')
    assert list(parts) == [7] and ids == [7, 8, 3] and end == [8, 3]
    assert _check({}, (), loudness) == ({}, [], [])
    assert _check({}, [8], loudness) == ({}, [8], [8])


def _lengths(core):
    """One stream that ends inside window 0, one that is an exact multiple of the core, one of 3 core + 1 frames."""
    return (max(1, core // 2), 2 * core, 3 * core + 1)


def _plan(F, core, context):
    """window_plan([F], core, context) without the utterance index.  window_plan refuses a core that is no multiple of 4,
    which the streams' row planning does not: for (5, 8) this is its documented rule, written out - window k owns [k core,
    min((k + 1) core, F)) and reads [max(0, k core - context), min(F, (k + 1) core + context))."""
    if core % 4 == 0:
        return [p[1:] for p in Dc.window_plan([F], core, context)]
    cores = [(k * core, min((k + 1) * core, F)) for k in range(-(-F // core))]
    return [(max(0, lo - context), min(F, lo + core + context), lo, hi) for lo, hi in cores]


def _play(core, context, rng, audio=False, emb=False, running=False, horizon=None, hop=160):
    """Drive stream_push_rows as StreamSession.push does over a random schedule of three streams -> per stream its rows
    and (with running) its forget entries; asserts a push's order and bookkeeping on the way."""
    F = _lengths(core)
    slots = rng.sample(range(3), 3)                      # (ids 10, 11, 12 in shuffled slots)
    st = [Dc._Stream(id=10 + u, slot=slots[u], emb=emb, seed=0, stats=None, from_audio=audio) for u in range(3)]
    live, rows, forget = {0, 1, 2}, [[] for _ in st], [[] for _ in st]
    pushes = 0
    while live:
        named = [u for u in sorted(live) if rng.random() < 0.8]
        ended = set()
        for u in named:
            left = F[u] - st[u].seen
            n = rng.randint(0, min(core, left))          # (0: a push that delivers nothing, or an end without a chunk)
            st[u].seen += n
            if st[u].seen == F[u] and rng.random() < 0.5:
                ended.add(st[u].id)
            if audio:
                st[u].final = Dc.stream_final_frames(st[u].seen, st[u].id in ended, hop)
        given = sorted((st[u] for u in named), key=lambda s: s.slot)
        before = {s.id: (s.done, s.norm_w) for s in given}
        got, fg = Dc.stream_push_rows(given, ended, core, context, running, horizon)
        pushes += 1
        assert all(isinstance(r, Dc.StreamRow) for r in got)
        assert [(r.stream, r.k) for r in got] == sorted((r.stream, r.k) for r in got)      # slot order, a stream's ascending
        assert {s.id: (s.done, s.norm_w) for s in given} == before                          # (it changes no record)
        assert len(fg) == (len(got) if running and emb else 0)
        for s in given:
            u = s.id - 10
            mine = [j for j, r in enumerate(got) if r.stream == s.slot]
            assert [got[j].k for j in mine] == list(range(s.done, s.done + len(mine)))
            assert all(got[j].in_hi <= s.complete for j in mine)
            rows[u] += [got[j] for j in mine]
            s.done += len(mine)                          # (what push does: done = k + 1 of the stream's last row ...)
            assert not mine or s.done == got[mine[-1]].k + 1
            if fg:
                forget[u] += [fg[j] for j in mine]
                if mine:
                    s.norm_w = fg[mine[-1]][3]           # (... and norm_w the w behind it)
            if s.id in ended:
                live.discard(u)
        assert pushes < 10000
    return F, rows, forget


@pytest.mark.parametrize("audio", (False, True))
@pytest.mark.parametrize("core,context", SIZES)
def test_push_rows_are_the_window_plan(core, context, audio):
    """Whatever the schedule - and with the loudness lag between the frames that arrived and those that count - a stream's
    rows, one push after the other, are window_plan's for its final length; last is set on exactly the final one."""
    rng = random.Random(1000 * core + 10 * context + audio)
    for _ in range(20):
        F, rows, _ = _play(core, context, rng, audio=audio)
        for u in range(3):
            plan = _plan(F[u], core, context)
            assert [tuple(r[2:6]) for r in rows[u]] == plan, (F[u], rows[u])
            assert [r.k for r in rows[u]] == list(range(len(plan)))
            assert [r.last for r in rows[u]] == [False] * (len(plan) - 1) + [True]
            assert all((r.frames, r.own_lo, r.own_hi) == (r[3] - r[2], r[4] - r[2], r[5] - r[2]) for r in rows[u])


@pytest.mark.parametrize("scale", (None, 1.0, 2.5))
@pytest.mark.parametrize("core,context", SIZES)
def test_forgetting_factors_are_running_horizon_rows_one_window_at_a_time(core, context, scale):
    """One running_horizon_rows call per stream and push gives, bit for bit, what a call per window with w threaded
    through gives; without a horizon that is decay 1, the frames up to the row's end, and the frames up to the core's."""
    horizon = None if scale is None else scale * core
    rng = random.Random(77 * core + context)
    for _ in range(20):
        F, rows, forget = _play(core, context, rng, emb=True, running=True, horizon=horizon)
        for u in range(3):
            assert len(forget[u]) == len(rows[u]) == len(_plan(F[u], core, context))
            w = None
            for r, f in zip(rows[u], forget[u]):
                (d,), (wt,), (bd,), w = Dc.running_horizon_rows([tuple(r[2:6])], horizon, w, core)
                assert f == (d, wt, bd, w) and all(type(v) is float for v in f), (r, f)
                if horizon is None:
                    assert f == (1.0, float(r.in_hi), float(r.in_hi), float(r.core_hi))
    _, rows, forget = _play(core, context, rng, emb=False, running=True, horizon=horizon)     # (no embedding: nothing carried)
    assert all(rows) and not any(forget)


def test_layout_takes_plain_tuples_and_stream_rows():
    core, context, fade, hop = 16, 8, 8, 4
    plain, named = Dc.stream_stitch_layout(2, hop, fade), Dc.stream_stitch_layout(2, hop, fade)
    seen, done = [0, 0], [0, 0]
    for pushed, ended in (((28, 9), ()), ((16, 16), ()), ((16, 3), (1,)), ((9, 0), (0,))):
        chunk = []
        for s in (0, 1):
            seen[s] += pushed[s]
            ready = Dc.stream_ready_rows(seen[s], s in ended, core, context, done[s])
            chunk += [(s, done[s] + j) + r + (s in ended and r[3] == seen[s],) for j, r in enumerate(ready)]
            done[s] += len(ready)
        assert chunk
        a, b = plain.batch(chunk, seen), named.batch([Dc.StreamRow(*r) for r in chunk], seen)
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        assert (plain.pending, plain.written) == (named.pending, named.written)
    assert done == [5, 2]


def test_constructor_sizes_without_a_device():
    cfg, hop = S.FULL_CONFIG, 160
    context = -(-Dc.receptive_field_frames(cfg) // 4) * 4
    lag = Dc.stream_loudness_lag(hop)
    assert (context, lag) == (36, 6)
    for loudness, cap, lag in (("given", Dc.stream_ring_frames(32, context, 32), 0),
                               ("audio", Dc.stream_loudness_ring_frames(32, context, 32, hop), lag)):
        got = Dc.StreamSession._check_args(cfg, hop, n_streams=3, core=32, context=None, max_push=32, loudness=loudness)
        assert (got["core"], got["context"], got["max_push"], got["cap"], got["lag"]) == (32, context, 32, cap, lag)
        assert got["_slice"] % 4 == 0 and 0 <= got["_slice"] - 32 * (cfg.in_channels + 1 + hop) < 4
        assert got["_down_elems"] == 3 * (cap * hop + 8 * (cap // 32 + 2))
        session = types.SimpleNamespace(**got)
        assert Dc.StreamSession.latency_frames.fget(session) == 32 + context + lag
        assert Dc.StreamSession.latency_frames_max.fget(session) == 64 + context + lag
    assert Dc.StreamSession._check_args(cfg, hop)["max_push"] == 32      # (max_push=None: the core)
    no_emb = dataclasses.replace(cfg, use_spk_emb=False)
    for c, kw, what in ((cfg, dict(norm="utterance"), "norm must be"),
                        (no_emb, dict(norm="running", context=36), "takes a speaker embedding"),
                        (cfg, dict(horizon=64), "needs norm"), (cfg, dict(norm="window", horizon=64), "needs norm"),
                        (cfg, dict(norm="running", horizon=31), "shorter than the core"),
                        (cfg, dict(loudness="raw"), "loudness must be"),
                        (cfg, dict(max_push=0), "max_push must be in"), (cfg, dict(max_push=2000), "max_push must be in"),
                        (cfg, dict(n_streams=0), "n_streams >= 1"), (cfg, dict(max_batch=0), "max_batch >= 1"),
                        (cfg, dict(core=30), "multiples of 4"), (cfg, dict(context=0, fade=8), "fade must be even")):
        with pytest.raises(ValueError, match=what):
            Dc.StreamSession._check_args(c, hop, **kw)
