"""The float64 reference of StreamSession(norm="running", horizon=H) (a helper, not a test): running_norm_ref's stream
reference with the forgetting rule of DESIGN.md 4.10 - at every norm point the carry is multiplied by the window's decay
before its core is added, and the window is normalised over decode.running_horizon_rows' weighted frame count.  The decay
is the ONE math.exp value the session uploads: both sides call running_horizon_rows."""
import numpy as np
import torch

from oracle import fastsvc_oracle as O
from svcc23_fastsvc_amd import decode as Dc

from running_norm_ref import NORM_POINTS


def stream_reference(wf, scales, ppg, exc, lft, emb, core, context, fade, norm="running", horizon=None):
    """ppg (1, C, F), exc and lft (1, 1, F hop), emb (E,) or None -> the stream's samples (F hop,) float64, and its rows.

    norm="window": every window by its own statistics (the oracle unchanged).  norm="running": at norm point p of window
    k >= 1, with u the FiLM-affined tensor of the row, m its columns per frame, A and L the (sum u, sum u^2) of its core and
    look-ahead columns and (decay, weight) = running_horizon_rows(window k, horizon, w_{k-1}),
        carry_p = decay carry_p + A, and the window is normalised by mean and biased variance (the oracle's eps) of the
        sums carry_p + L over N = weight m columns.
    horizon=None: decay is exactly 1.0 and weight is in_hi - running_norm_ref.stream_reference's bits.  Window 0 owns its
    whole row: it keeps the oracle's own InstanceNorm and only feeds the carry."""
    assert norm in ("window", "running")
    F = int(ppg.shape[-1])
    hop = int(np.prod(list(scales)))
    rows = Dc.window_plan([F], core, context)
    state = dict(carry=[None] * NORM_POINTS, call=0, row=None)
    plain = O._instance_norm

    def running_norm(u):
        p = state["call"]
        state["call"] += 1
        assert p < NORM_POINTS and u.shape[0] == 1 and u.dtype == torch.float64
        k, in_lo, in_hi, lo, hi, decay, weight = state["row"]
        m = u.shape[-1] // (in_hi - in_lo)
        assert m * (in_hi - in_lo) == u.shape[-1]
        c0, c1 = (lo - in_lo) * m, (hi - in_lo) * m
        a = torch.stack([u[..., c0:c1].sum(dim=-1), (u[..., c0:c1] ** 2).sum(dim=-1)])
        carry = a if state["carry"][p] is None else state["carry"][p] * decay + a
        state["carry"][p] = carry
        if k == 0:
            return plain(u)
        s = carry + torch.stack([u[..., c1:].sum(dim=-1), (u[..., c1:] ** 2).sum(dim=-1)])
        n = float(weight * m)
        mean = (s[0] / n).unsqueeze(-1)
        var = (s[1] / n).unsqueeze(-1) - mean * mean
        return (u - mean) / torch.sqrt(var + O.IN_EPS)

    ys = []
    if norm == "running" and emb is not None:
        O._instance_norm = running_norm
    w = None
    try:
        for k, (_, in_lo, in_hi, lo, hi) in enumerate(rows):
            (decay,), (weight,), _, w = Dc.running_horizon_rows([(in_lo, in_hi, lo, hi)], horizon, w, core)
            state["row"], state["call"] = (k, in_lo, in_hi, lo, hi, decay, weight), 0
            y = O.forward_dedup(wf, scales, ppg[:, :, in_lo:in_hi], exc[:, :, in_lo * hop: in_hi * hop],
                                lft[:, :, in_lo * hop: in_hi * hop], None if emb is None else np.asarray(emb)[None],
                                dtype=torch.float64).numpy()[0, 0]
            if O._instance_norm is running_norm:
                assert state["call"] == NORM_POINTS, state["call"]
            ys.append(y)
    finally:
        O._instance_norm = plain
    return Dc.stitch_windows(ys, rows, hop, fade)[0].astype(np.float64), rows
