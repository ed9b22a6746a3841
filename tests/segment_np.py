"""numpy restatement of ground-truth-free instance inference (ReSeg.segment), written from the procedure's text and
not from the kernels.  A helper module for tests/test_segment_ref.py and tests/test_gpu_segment.py.

    labels = 0 (uint8 [B,L]);  count = 0 (int32 [B]);  remaining = fg
    for t in 0 .. max_objects-1:
        active[b] = any(remaining[b]);  stop when no image is active
        s_t[b]    = first arg-max of merge[b,p] over p with remaining[b,p]      (0 for an inactive image)
        pred      = decode(s_t)                                                 [B,L,2] logits
        claim[b,p] = remaining[b,p] and (pred[b,p,1] > pred[b,p,0] or p == s_t[b]),  active images only
        labels[b,p] = count[b] + 1 where claim;  count[b] += 1 (active images);  remaining &= not claim

Arg-max rules: the first maximum wins; NaN never wins - it ranks as -inf; if no remaining pixel scores above -inf
(all of them NaN or -inf) the first remaining pixel is the point, so the point of an active image is always one of its
remaining pixels, it is always claimed, and every iteration of an active image removes at least one pixel.
`>` on a NaN logit is false.  Labels are uint8: an image that holds 255 instances claims nothing more.

`flaws` switches on one deliberate mistake at a time (what a wrong kernel would likely do), so that the CPU tests can show
that the cases they use tell such kernels apart."""
import numpy as np

FLAWS = ("last_max", "no_forced_point", "ge", "overwrite", "relabel_inactive")


def masked_first_argmax(score, mask, flaws=()):
    """Index of the first maximum of score over mask (1-D arrays), or -1 when the mask is empty."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return -1
    v = np.asarray(score, dtype=np.float64)[idx].copy()
    v[np.isnan(v)] = -np.inf
    best = v.max()
    hits = idx[v == best]
    return int(hits[-1] if "last_max" in flaws else hits[0])


def seg_begin(sem, merge, flaws=()):
    """State after isa_seg_begin.  sem, merge: [B,L]."""
    sem = np.asarray(sem)
    B, L = sem.shape
    st = dict(labels=np.zeros((B, L), np.uint8), count=np.zeros(B, np.int32), s_t=np.zeros(B, np.int32),
              active=np.zeros(B, np.int32))
    _next_points(st, sem, merge, flaws)
    return st


def _next_points(st, sem, merge, flaws):
    remaining = (np.asarray(sem) > 0.5) & (st["labels"] == 0)
    for b in range(remaining.shape[0]):
        p = masked_first_argmax(merge[b], remaining[b], flaws)
        st["active"][b] = 1 if p >= 0 else 0
        st["s_t"][b] = max(p, 0)
    st["any"] = int(st["active"].any())


def seg_claim(st, pred, sem, merge, s_t=None, flaws=()):
    """One claim step, in place, as isa_seg_claim: pred [B,L,2] are the logits decoded for the points s_t (default:
    the state's own).  Afterwards st holds the next points."""
    pred = np.asarray(pred, dtype=np.float64)
    s_t = st["s_t"] if s_t is None else np.asarray(s_t)
    B, L = st["labels"].shape
    for b in range(B):
        act = st["active"][b] != 0 and st["count"][b] < 255
        if not act and "relabel_inactive" not in flaws:
            continue
        remaining = (np.asarray(sem[b]) > 0.5) & (st["labels"][b] == 0)
        if "overwrite" in flaws:
            remaining = np.asarray(sem[b]) > 0.5
        with np.errstate(invalid="ignore"):
            wants = pred[b, :, 1] >= pred[b, :, 0] if "ge" in flaws else pred[b, :, 1] > pred[b, :, 0]
        if "no_forced_point" not in flaws:
            wants = wants.copy()
            wants[int(s_t[b])] = True
        claim = remaining & wants
        st["labels"][b][claim] = st["count"][b] + 1
        st["count"][b] += 1
    _next_points(st, sem, merge, flaws)
    return st


def segment_loop(fg, merge, decode, max_objects=32, injected_s_t=None, flaws=()):
    """The whole procedure.  decode(s_t [B] int) -> logits [B,L,2].  Returns (labels uint8 [B,L], count int32 [B],
    trace) with trace[t] = dict(s_t, active, claimed [B] pixel counts)."""
    st = seg_begin(fg, merge, flaws)
    trace = []
    iters = max_objects if injected_s_t is None else len(injected_s_t)
    for t in range(iters):
        if injected_s_t is None and not st["any"]:
            break
        s_t = st["s_t"].copy() if injected_s_t is None else np.asarray(injected_s_t[t]).astype(np.int32)
        active = st["active"].copy()
        before = (st["labels"] != 0).sum(1)
        seg_claim(st, decode(s_t), fg, merge, s_t, flaws)
        trace.append(dict(s_t=s_t, active=active, claimed=(st["labels"] != 0).sum(1) - before))
    return st["labels"], st["count"], trace
