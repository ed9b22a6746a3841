"""The rules of isa_sem_confusion / isa_sem_scores restated in numpy (include/isa_kernels.h), for the tests to compare with.

class_map(logits, K): arg-max over channels 0..K-1 of logits [..., ld]; the first maximum wins, NaN counts as the maximum
    (so the first NaN channel wins: torch.argmax, isa_chan_argmax), all -inf gives class 0; channels >= K never take part.
confusion(labels, pred, K) -> (conf int64 [n,K,K], oob int64 [n]): conf[i][t][p] pixels of image i with label t and
    prediction p; a pixel with label >= K is counted in oob[i] instead.
scores(conf) -> float64 [..., 4+2K]: 0 pixel accuracy, 1 mean IoU and 2 mean Dice over the classes with gt + pr - tp > 0
    (summed in class order), 3 their number, then IoU[K] and Dice[K]; NaN for a class absent from both maps, for the
    means when there is no class, and for the accuracy of an empty matrix.  Every per-class value is one float64 division
    of exact integers."""
import numpy as np

NAN = float("nan")


def class_map(logits, K):
    x = np.asarray(logits)[..., :K].astype(np.float64)             # (fp32 and bf16 values are exact in float64)
    nan = np.isnan(x)
    first_nan = np.argmax(nan, axis=-1)
    # np.argmax returns the first maximum; NaN must not take part in it (np.argmax would pick the first NaN, which is the
    # rule, but say so explicitly instead of leaning on it)
    plain = np.argmax(np.where(nan, -np.inf, x), axis=-1)
    return np.where(nan.any(axis=-1), first_nan, plain).astype(np.uint8)


def confusion(labels, pred, K):
    labels, pred = np.asarray(labels), np.asarray(pred)
    n = labels.shape[0]
    lab, pr = labels.reshape(n, -1).astype(np.int64), pred.reshape(n, -1).astype(np.int64)
    assert lab.shape == pr.shape and (pr < K).all()
    conf, oob = np.zeros((n, K, K), np.int64), np.zeros(n, np.int64)
    for i in range(n):
        ok = lab[i] < K
        oob[i] = int((~ok).sum())
        conf[i] = np.bincount(lab[i][ok] * K + pr[i][ok], minlength=K * K).reshape(K, K)
    return conf, oob


def scores(conf):
    conf = np.asarray(conf, np.int64)
    if conf.ndim == 3:
        return np.stack([scores(c) for c in conf]) if len(conf) else np.zeros((0, 4 + 2 * conf.shape[1]))
    K = conf.shape[0]
    out = np.full(4 + 2 * K, NAN, np.float64)
    si = sd = 0.0
    cnt = 0
    for c in range(K):
        tp, gt, pr = int(conf[c, c]), int(conf[c].sum()), int(conf[:, c].sum())
        if gt + pr - tp > 0:
            out[4 + c] = np.float64(tp) / np.float64(gt + pr - tp)
            out[4 + K + c] = np.float64(2 * tp) / np.float64(gt + pr)
            si += out[4 + c]
            sd += out[4 + K + c]
            cnt += 1
    total, trace = int(conf.sum()), int(np.trace(conf))
    if total:
        out[0] = np.float64(trace) / np.float64(total)
    if cnt:
        out[1], out[2] = si / cnt, sd / cnt
    out[3] = cnt
    return out
