"""CPU tests of the live-stream decode's host side (decode.StreamSession): which windows are ready, the incremental
stitch layout against stitch_layout, the latency rule, the ring capacity in a host model, and the carried sine phase
against the whole-utterance scan in numpy."""
import random

import numpy as np
import pytest

from svcc23_fastsvc_amd import decode as Dc

FRAMES = (1, 9, 32, 33, 52, 64, 68, 100, 160)
SIZES = ((32, 36), (16, 8), (32, 0))        # (core, context)
PUSHES = (0, 1, 3, 4, 7, 33, 45, 48)


def _schedules(F, rng, n=6):
    """Push schedules for a stream of F frames: lists of (frames, ended).  Random sizes (0 included); the end comes with
    the last frames or in a call of its own after them; plus frame by frame, and everything at once."""
    out = [[(1, i == F - 1) for i in range(F)], [(F, True)], [(F, False), (0, True)]]
    for _ in range(n):
        sched, left = [], F
        while left:
            k = min(rng.choice(PUSHES), left)
            left -= k
            sched.append((k, False))
        if rng.random() < 0.5:
            sched[-1] = (sched[-1][0], True)
        else:
            sched.append((0, True))
        out.append(sched)
    return out


def _run(F, core, context, fade, sched, hop=4, stream=0, n_streams=1):
    """Drive stream_ready_rows and the incremental layout over a schedule -> (rows, batches of row indices, the layout's
    per-batch dicts, per push the (first, last) sample the push returned or None)."""
    lay = Dc.stream_stitch_layout(n_streams, hop, fade)
    seen = done = 0
    rows, batches, dicts, returned = [], [], [], []
    for k, ended in sched:
        seen += k
        ready = Dc.stream_ready_rows(seen, ended, core, context, done)
        if not ready:
            returned.append(None)
            continue
        chunk = [(stream, done + j) + r + (ended and r[3] == seen,) for j, r in enumerate(ready)]
        seens = [0] * n_streams
        seens[stream] = seen
        d = lay.batch(chunk, seens)
        batches.append(list(range(done, done + len(ready))))
        rows += [(0,) + r for r in ready]
        dicts.append(d)
        done += len(ready)
        returned.append((d["runs"][0][1], d["runs"][-1][2]))
    return rows, batches, dicts, returned


@pytest.mark.parametrize("core,context", SIZES)
def test_ready_rows_are_the_window_plan(core, context):
    """Whatever the schedule - pushes of 0 frames, the end with the last frames or alone, an end exactly on a core
    boundary (F = 32, 64) - a stream's rows are window_plan's for its final length, each produced once, and no window
    runs before everything it reads has arrived."""
    rng = random.Random(core * 100 + context)
    for F in FRAMES:
        plan = Dc.window_plan([F], core, context)
        for sched in _schedules(F, rng):
            seen = done = 0
            rows = []
            for k, ended in sched:
                seen += k
                ready = Dc.stream_ready_rows(seen, ended, core, context, done)
                for _, in_hi, _, hi in ready:
                    assert in_hi <= seen and (ended or in_hi == hi + context)
                rows += [(0,) + r for r in ready]
                done += len(ready)
                assert not Dc.stream_ready_rows(seen, ended, core, context, done)
            assert rows == plan, (F, sched)
    assert Dc.stream_ready_rows(0, True, core, context, 0) == []            # (a stream that ends without a frame)


@pytest.mark.parametrize("core,context,fade", [(32, 36, 8), (16, 8, 8), (16, 8, 2), (32, 36, 0), (32, 0, 0)])
def test_incremental_layout_is_stitch_layout_with_every_push_a_batch(core, context, fade):
    """Modes, FROM_Y sources, n_samples / core_lo / core_hi, dst_off, runs, total and width of every push equal
    stitch_layout's for the whole stream's rows with the pushes as batches; the staged zones live in the stream's two
    slots, a slot is read by the window after the one that wrote it, and NO batch holds a row that stages into the slot
    another of its rows reads (the rows of one stitch launch are not ordered) - batches that both read and stage do
    occur; the runs cover [0, F hop) once each, in order."""
    rng = random.Random(core + context + fade)
    hop, n_streams, stream = 6, 3, 2
    both = 0
    for F in FRAMES:
        for sched in _schedules(F, rng):
            rows, batches, dicts, _ = _run(F, core, context, fade, sched, hop, stream, n_streams)
            assert rows == Dc.window_plan([F], core, context)
            ref, _ = Dc.stitch_layout(rows, batches, hop, fade)
            assert len(ref) == len(dicts)
            staged = {}
            pos, k = 0, 0
            for d, r in zip(dicts, ref):
                for key in ("n_samples", "core_lo", "core_hi", "left_mode", "right_mode", "dst_off", "total", "width", "half"):
                    assert d[key] == r[key], (key, F, sched)
                assert [run[1:] for run in d["runs"]] == [run[1:] for run in r["runs"]]
                assert d["utt"] == [stream] * len(d["utt"])
                both += _no_slot_is_read_and_staged_in_one_batch(d, fade * hop)
                for j in range(len(d["utt"])):
                    if d["right_mode"][j] == 3:
                        assert d["right_src"][j] == r["right_src"][j]
                    if d["left_mode"][j] == 2:                           # FROM_STAGE: the slot window k - 1 staged
                        assert staged.pop(k - 1) == d["left_src"][j]
                    if d["right_mode"][j] == 1:                          # STAGE
                        assert d["right_src"][j] in ((2 * stream) * fade * hop, (2 * stream + 1) * fade * hop)
                        assert d["right_src"][j] + fade * hop <= Dc.stream_stitch_layout(n_streams, hop, fade).stage_elems
                        staged[k] = d["right_src"][j]
                    assert d["runs"][j][1] == pos                        # the runs follow each other ...
                    pos = d["runs"][j][2]
                    k += 1
            assert pos == F * hop and not staged                         # ... and end with the stream
    assert both > 0 or not fade or core == 32                            # (core 16 with pushes of 33 - 48 frames: such batches exist)


def _no_slot_is_read_and_staged_in_one_batch(d, fh):
    """-> 1 if the batch both reads and stages slots (and they are disjoint), else 0."""
    reads = [d["left_src"][j] for j in range(len(d["utt"])) if d["left_mode"][j] == 2]
    writes = [d["right_src"][j] for j in range(len(d["utt"])) if d["right_mode"][j] == 1]
    assert len(set(writes)) == len(writes)
    for r in reads:
        for w in writes:
            assert r + fh <= w or w + fh <= r, (reads, writes)
    return int(bool(reads) and bool(writes))


@pytest.mark.parametrize("max_batch", [1, 2, 3])
def test_a_push_split_into_forwards_is_stitch_layout_too(max_batch):
    """Three streams flush 7, 4 and 10 windows in one push that is cut into forwards of `max_batch` rows, after one
    window of each ran alone: every forward's fields are stitch_layout's for those batches, and no forward stages into a
    slot that one of its rows reads."""
    core, context, fade, hop = 16, 8, 8, 6
    frames = [100, 52, 160]
    plan = Dc.window_plan(frames, core, context)
    first = {u: next(i for i, r in enumerate(plan) if r[0] == u) for u in range(3)}
    lay = Dc.stream_stitch_layout(3, hop, fade)
    rows, batches = [], []
    for u in range(3):                                   # window 0 of every stream, with 24 frames seen
        r = Dc.stream_ready_rows(core + context, False, core, context, 0)
        assert len(r) == 1
        rows.append([(u, 0) + r[0] + (False,)])
        batches.append([first[u]])
    flush = []
    for u, F in enumerate(frames):
        ready = Dc.stream_ready_rows(F, True, core, context, 1)
        flush += [(u, 1 + j) + r + (r[3] == F,) for j, r in enumerate(ready)]
    for c0 in range(0, len(flush), max_batch):
        rows.append(flush[c0: c0 + max_batch])
        batches.append([first[r[0]] + r[1] for r in rows[-1]])
    seen = [core + context] * 3
    dicts = [lay.batch(chunk, seen) for chunk in rows[:3]]
    dicts += [lay.batch(chunk, frames) for chunk in rows[3:]]
    ref, _ = Dc.stitch_layout(plan, batches, hop, fade)
    both = 0
    for d, r in zip(dicts, ref):
        for key in ("n_samples", "core_lo", "core_hi", "left_mode", "right_mode", "dst_off", "runs", "total", "width", "half", "utt"):
            assert d[key] == r[key], key
        both += _no_slot_is_read_and_staged_in_one_batch(d, fade * hop)
    assert both > 0 or max_batch == 1
    assert lay.pending == [None] * 3


def test_layout_refuses_a_window_whose_neighbour_never_staged():
    lay = Dc.stream_stitch_layout(1, 4, 8)
    with pytest.raises(ValueError):
        lay.batch([(0, 1, 0, 100, 32, 64, False)], [100])
    assert lay.pending == [None]                                         # (a refused batch changes nothing)
    with pytest.raises(ValueError):
        Dc.stream_stitch_layout(1, 4, 3)


def _return_frame(t, F, core, context, fade):
    """The frame whose push returns the samples of frame t (the docstring's rule), with the end at frame F - 1."""
    k = t // core
    r = (k + 1) * core + context - 1
    if t % core >= core - fade // 2:
        r = (k + 2) * core + context - 1
    return min(r, F - 1)


@pytest.mark.parametrize("core,context,fade", [(32, 36, 8), (32, 36, 0), (16, 8, 4)])
def test_latency_rule_for_every_sample(core, context, fade):
    """A 160-frame stream pushed frame by frame (the end with the last frame): every sample comes back with exactly the
    frame the rule names."""
    F, hop = 160, 4
    sched = [(1, i == F - 1) for i in range(F)]
    _, _, _, returned = _run(F, core, context, fade, sched, hop)
    got = np.full(F * hop, -1)
    for frame, run in enumerate(returned):
        if run is not None:
            assert (got[run[0]: run[1]] == -1).all()
            got[run[0]: run[1]] = frame
    want = np.repeat([_return_frame(t, F, core, context, fade) for t in range(F)], hop)
    assert np.array_equal(got, want)
    assert (want - np.repeat(np.arange(F), hop)).max() <= 2 * core + context - 1


@pytest.mark.parametrize("core,context,max_push", [(32, 36, 32), (32, 36, 48), (16, 8, 1), (16, 8, 45), (32, 0, 7), (4, 4, 3)])
def test_ring_capacity_keeps_every_frame_a_window_still_needs(core, context, max_push):
    """A host model of the ring: frame p is written to index p % cap, and every window that runs finds its frames
    there - for any schedule whose pushes are at most max_push frames."""
    cap = Dc.stream_ring_frames(core, context, max_push)
    assert cap % 4 == 0 and core + 2 * context + max_push <= cap < core + 2 * context + max_push + 4
    rng = random.Random(cap)
    for F in (1, 9, 52, 160, 333):
        for _ in range(8):
            ring = np.full(cap, -1)
            seen = done = 0
            while True:
                k = min(rng.choice([0, 1, 3, max_push, max_push, rng.randint(0, max_push)]), F - seen)
                ring[np.arange(seen, seen + k) % cap] = np.arange(seen, seen + k)
                seen += k
                ended = seen == F and rng.random() < 0.7
                for in_lo, in_hi, _, _ in Dc.stream_ready_rows(seen, ended, core, context, done):
                    assert seen - cap <= in_lo and in_hi <= seen
                    assert np.array_equal(ring[np.arange(in_lo, in_hi) % cap], np.arange(in_lo, in_hi))
                    done += 1
                if ended:
                    break


def _excitation_model(f0, hop, sample_rate, sine_amp, chunks=None):
    """The numpy model of the noise-free sine excitation (float32 samples), as the kernels compute it.  ``chunks=None``:
    csrc/fastsvc_signal.hip on the whole f0 - ``frame_phase_kernel``'s scan (256 segments of ``ceil(F / 256)`` frames,
    their sums scanned modulo 1, then the recurrence inside each segment) and ``synth_kernel``'s closed form.
    ``chunks``: csrc/fastsvc_stream.hip - the recurrence ``c <- frac(c + hop rad)`` carried from chunk to chunk.  Both in
    float64 with rad in float32; they agree bit for bit while every add is exact."""
    f0 = np.asarray(f0, dtype=np.float32).reshape(-1)
    F, hop = f0.size, int(hop)
    rad = np.fmod(f0 / np.float32(sample_rate), np.float32(1.0)).astype(np.float32)
    step = np.float64(hop) * rad.astype(np.float64)
    cf = np.zeros(F, dtype=np.float64)
    if chunks is None:
        per = -(-F // 256)
        part = [np.float64(0.0)] * 256
        for t in range(256):
            s = np.float64(0.0)
            for i in range(t * per, min(F, t * per + per)):
                s = s + step[i]
            part[t] = s
        run = np.float64(0.0)
        for t in range(256):
            v, part[t] = part[t], run
            run = run + v
            run = run - np.floor(run)
        for t in range(256):
            run = part[t]
            for i in range(t * per, min(F, t * per + per)):
                cf[i] = run
                run = run + step[i]
                run = run - np.floor(run)
    else:
        if sum(int(n) for n in chunks) != F:
            raise ValueError("the chunks must add up to the frames of f0")
        c, i = np.float64(0.0), 0                        # (c is what the push stores between the chunks)
        for n in chunks:
            for _ in range(int(n)):
                cf[i] = c
                c = c + step[i]
                c = c - np.floor(c)
                i += 1
    j = np.arange(1, hop + 1, dtype=np.float64)
    ph = cf[:, None] + j[None, :] * rad.astype(np.float64)[:, None]
    ph = ph - np.floor(ph)
    vuv = (f0 > 0).astype(np.float32)
    two_pi = np.float64(6.283185307179586476925286766559)
    return (vuv[:, None] * np.sin(ph * two_pi).astype(np.float32) * np.float32(sine_amp)).astype(np.float32).reshape(-1)


def _f0(F, seed):
    """F0 in {0} u [50, 1000] Hz as float32: voiced and unvoiced stretches of random lengths."""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(50.0, 1000.0, F).astype(np.float32)
    f0[0], f0[-1] = 50.0, 1000.0
    i = 0
    while i < F:
        n = int(rng.integers(1, 40))
        if rng.random() < 0.35:
            f0[i: i + n] = 0.0
        i += n
    return f0


@pytest.mark.parametrize("F,hop", [(300, 160), (2400, 160), (700, 60), (24000, 160)])
def test_carried_phase_equals_the_whole_utterance_scan_in_numpy(F, hop):
    """The numpy model of the streamed excitation (the recurrence carried across irregular chunks) equals the numpy
    model of frame_phase_kernel + synth_kernel on the whole f0, bit for bit: every float64 add of hop x rad is exact."""
    f0 = _f0(F, F + hop)
    assert (f0 == 0).any() and (f0 > 0).any()
    whole = _excitation_model(f0, hop, 24000.0, 0.1)
    rng = random.Random(F)
    for chunks in ([1] * F, [F], None):
        if chunks is None:
            chunks, left = [], F
            while left:
                chunks.append(min(rng.choice(PUSHES), left))
                left -= chunks[-1]
        got = _excitation_model(f0, hop, 24000.0, 0.1, chunks=chunks)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    assert np.abs(whole).max() > 0.09 and not whole.reshape(F, hop)[f0 == 0].any()


def test_the_library_refuses_on_the_host_and_names_the_stream():
    """fastsvc_stream_push / fastsvc_stream_assemble validate everything before they enqueue anything, so their
    refusals need no GPU: FASTSVC_E_INVALID (-1), with the stream or row and the reason in fastsvc_last_error()."""
    import ctypes
    import svcc23_fastsvc_amd as A
    from svcc23_fastsvc_amd.build import build
    build()
    lib = A.load_library()
    i32, i64, u64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    fake = lambda k: vp(0x10000 * (k + 1))               # noqa: E731  (never dereferenced: every call below is refused)
    C, hop, cap, max_push, n_streams = 4, 4, 16, 8, 3

    def push(streams=(0, 2), n=(8, 0), up_off=(0, 0), pos=(0, 0), upload_elems=72, max_push=max_push, cap=cap, upload=fake(0)):
        S = len(streams)
        return lib.fastsvc_stream_push(upload, upload_elems, S, (i32 * S)(*streams), (i32 * S)(*n), (i64 * S)(*up_off), (i64 * S)(*pos),
                                       (i32 * S)(*[1] * S), (i32 * S)(*[0] * S), (u64 * S)(*[0] * S), fake(1), fake(2), fake(3), fake(4),
                                       n_streams, cap, max_push, C, hop, ctypes.c_float(24000.0), ctypes.c_float(0.1),
                                       ctypes.c_float(0.0), None)
    for kw, words in ((dict(n=(9, 0)), ("stream 0", "9 frames", "max_push")), (dict(n=(0, -1)), ("stream 2",)),
                      (dict(up_off=(1, 0)), ("stream 0", "upload buffer")), (dict(upload_elems=71), ("stream 0", "upload buffer")),
                      (dict(streams=(0, 3)), ("stream 3",)), (dict(streams=(2, 2)), ("stream 2", "twice")),
                      (dict(pos=(0, -5)), ("stream 2", "position")), (dict(max_push=17), ("max_push",)),
                      (dict(max_push=2000, cap=4096), ("max_push",)), (dict(cap=18), ("multiple of 4",)),
                      (dict(upload=None), ("null",))):
        assert push(**kw) == -1, kw
        msg = lib.fastsvc_last_error().decode()
        assert msg.startswith("fastsvc_stream_push") and all(w in msg for w in words), (kw, msg)

    def assemble(streams=(0,), first=(36,), frames=(4,), pos=(100, 171, 0), width=60):
        R = len(streams)
        return lib.fastsvc_stream_assemble(fake(1), fake(2), fake(3), n_streams, 64, (i64 * 3)(*pos), (i32 * R)(*streams), (i64 * R)(*first),
                                           (i32 * R)(*frames), fake(4), fake(5), fake(6), R, C, hop, width, None)
    for kw, words in ((dict(first=(35,)), ("row 0", "not retained")), (dict(first=(97,)), ("row 0", "not retained")),
                      (dict(streams=(0, 1), first=(36, 106), frames=(4, 1)), ("row 1", "not retained")),
                      (dict(streams=(2,), first=(0,), frames=(1,)), ("row 0", "not retained")),
                      (dict(streams=(3,)), ("row 0", "stream 3")), (dict(frames=(61,)), ("row 0", "61 frames")),
                      (dict(first=(-1,)), ("row 0",)), (dict(width=0), ("width",))):
        assert assemble(**kw) == -1, kw
        msg = lib.fastsvc_last_error().decode()
        assert msg.startswith("fastsvc_stream_assemble") and all(w in msg for w in words), (kw, msg)
    assert lib.fastsvc_stream_launch_count(0) == 0 and lib.fastsvc_stream_launch_count(64) == 1 and lib.fastsvc_stream_launch_count(65) == 2
    # a push of nothing is accepted and enqueues nothing
    assert push(n=(0, 0)) == 0
