#!/usr/bin/env python3
"""Time of clustering an instance embedding into instances on the device (ReSeg.cluster_embedding: isa_cluster_meanshift,
isa_cluster_kmeans) against the same formulas in torch ops, against ReSeg.segment on images of the same size and, where
scikit-learn imports, against sklearn's KMeans on the host - what the reference's Prediction.cluster calls.

Inputs already on the device: an embedding NHWC [B,H,W,C = 24] (bf16, then fp32) of 8 planted instances an image (centres at
pairwise distance 3, noise 0.1 a channel, 8 x 8 blocks) and a uint8 foreground map.
  (a) mean-shift : bandwidth 1.5, 3 shifts, max_objects 8 (what a caller who knows the bound passes) and 32 (the default);
  (b) k-means    : 8 clusters, farthest-point init, 10 Lloyd iterations;
  (c) torch      : the same k-means (init, iterations, direct-form distances as broadcast differences, one-hot matmul for the
                   means) and the same mean-shift (a host loop over objects with one read-back per object to stop);
  (d) segment    : ReSeg.segment(max_objects=8) of a bf16 instance model on random images of the same size: a decoder pass
                   per object, the path the clustering is an alternative to (weights random: the time is what is compared);
  (e) sklearn    : KMeans(init=the same centres, n_init=1, algorithm='lloyd', tol=0, max_iter=10) over one image's
                   foreground on the host, times B (the copy to the host not counted).
(a)-(c) are called alternately, --calls times each after --warmup, every call timed with events of its own; the median is
reported.  No threshold: the script reports.  Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import isa_amd  # noqa: F401,E402
from isa_amd.engine import Act  # noqa: E402
from isa_amd.labelmaps import LabelOps  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402

K_OBJ, BW, SHIFTS, ITERS = 8, 1.5, 3, 10


def timed_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(fns, calls, warmup):
    """Median ms of each function, called in turn."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for i, f in enumerate(fns):
            ts[i].append(timed_ms(f))
    return [statistics.median(t) for t in ts]


def sqdist(x, c):
    """[B, L, K] direct-form squared distances of x [B, L, C] to c [B, K, C]."""
    return torch.stack([((x - c[:, k:k + 1]) ** 2).sum(2) for k in range(c.shape[1])], 2)


def torch_kmeans(x, fg, K, iters):
    """x [B, L, C] fp32, fg [B, L] bool.  Farthest-point init and Lloyd with the rules of isa_cluster_kmeans."""
    B, L, C = x.shape
    big = torch.iinfo(torch.int64).max
    first = torch.where(fg, torch.arange(L, device=x.device)[None], big).min(1).values
    cen = [x[torch.arange(B), first]]
    dmin = torch.where(fg, ((x - cen[0][:, None]) ** 2).sum(2), -1.0)
    for _ in range(1, K):
        j = dmin.argmax(1)
        cen.append(x[torch.arange(B), j])
        dmin = torch.where(fg, torch.minimum(dmin, ((x - cen[-1][:, None]) ** 2).sum(2)), -1.0)
    c = torch.stack(cen, 1)
    for i in range(iters + 1):
        lab = sqdist(x, c).argmin(2)
        if i == iters:
            break
        onehot = torch.nn.functional.one_hot(lab, K).float() * fg[..., None]
        n = onehot.sum(1)
        c = torch.where(n[..., None] > 0, torch.bmm(onehot.transpose(1, 2), x) / n.clamp_min(1)[..., None], c)
    return torch.where(fg, lab + 1, 0).to(torch.uint8), c


def torch_meanshift(x, fg, bw, shifts, max_objects):
    """The greedy mean-shift of isa_cluster_meanshift (min_pixels 1) in torch ops, all images advancing together."""
    B, L, C = x.shape
    labels = torch.zeros((B, L), dtype=torch.uint8, device=x.device)
    idx = torch.arange(L, device=x.device)[None]
    rows = torch.arange(B, device=x.device)
    k = torch.zeros(B, dtype=torch.int64, device=x.device)
    for _ in range(max_objects):
        free = fg & (labels == 0)
        live = free.any(1)
        if not bool(live.any()):                                   # the read-back a host loop needs to stop
            break
        s = torch.where(free, idx, L).min(1).values.clamp_max(L - 1)
        c = x[rows, s]
        for _ in range(shifts):
            S = free & (((x - c[:, None]) ** 2).sum(2) <= bw * bw)
            n = S.sum(1, keepdim=True)
            c = torch.where(n > 0, (x * S[..., None]).sum(1) / n.clamp_min(1), c)
        S = free & ((((x - c[:, None]) ** 2).sum(2) <= bw * bw) | (idx == s[:, None]))
        k = k + live
        labels = torch.where(S & live[:, None], k[:, None].to(torch.uint8), labels)
    return labels, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-segment", action="store_true", help="skip ReSeg.segment")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cluster.py needs the GPU"
    B, S, C = opt.batch, opt.size, opt.channels
    lines = ["cluster bench: %s, B=%d, %d x %d, C=%d, %d planted instances an image; median of %d alternating calls after %d "
             "warm-up, one event pair per call" % (torch.cuda.get_device_name(0), B, S, S, C, K_OBJ, opt.calls, opt.warmup)]
    m = LabelOps()
    g = torch.Generator(device="cuda").manual_seed(5)
    truth = torch.randint(0, K_OBJ + 1, (B, S // 8, S // 8), generator=g, device="cuda", dtype=torch.int32)
    truth = truth.repeat_interleave(8, 1).repeat_interleave(8, 2).long().contiguous()
    q, _ = torch.linalg.qr(torch.randn((C, C), generator=g, device="cuda"))
    centres = torch.cat([torch.zeros((1, C), device="cuda"), q[:K_OBJ] * (3.0 / 2.0 ** 0.5)])
    base = torch.randn((B, S, S, C), generator=g, device="cuda") * 0.1 + centres[truth]
    fg = (truth > 0).to(torch.uint8).contiguous()
    n_obj = torch.full((B,), K_OBJ, dtype=torch.int32, device="cuda")
    for dtype in (torch.bfloat16, torch.float32):
        emb = base.to(dtype).contiguous()
        a = Act(emb, 0, C)
        x32 = emb.float().reshape(B, -1, C)
        fgb = fg.view(B, -1) != 0
        res = {}

        def ms8():
            res["ms8"] = m.cluster_embedding(a, fg, bandwidth=BW, shifts=SHIFTS, max_objects=K_OBJ)

        def ms32():
            res["ms32"] = m.cluster_embedding(a, fg, bandwidth=BW, shifts=SHIFTS)

        def km():
            res["km"] = m.cluster_embedding(a, fg, method="kmeans", n_objects=n_obj, iters=ITERS, max_objects=K_OBJ)

        def t_km():
            res["t_km"] = torch_kmeans(x32, fgb, K_OBJ, ITERS)

        def t_ms():
            res["t_ms"] = torch_meanshift(x32, fgb, BW, SHIFTS, K_OBJ)

        t = alternate([ms8, ms32, km, t_km, t_ms], opt.calls, opt.warmup)
        same_km = float((res["km"]["labels"].view(B, -1) == res["t_km"][0]).float().mean())
        same_ms = float((res["ms8"]["labels"].view(B, -1) == res["t_ms"][0]).float().mean())
        found = res["ms32"]["n_objects"].tolist()
        lines.append("%-8s (a) mean-shift max_objects=8 %8.3f ms, =32 %8.3f ms   (b) k-means %8.3f ms   (c) torch k-means %8.3f ms "
                     "(%.1fx), torch mean-shift %8.3f ms (%.1fx)   labels equal to torch's: k-means %.4f, mean-shift %.4f; "
                     "objects found %d..%d; one pass over the embedding = %.1f MB"
                     % (str(dtype)[6:], t[0], t[1], t[2], t[3], t[3] / t[2], t[4], t[4] / t[0], same_km, same_ms, min(found),
                        max(found), B * S * S * C * emb.element_size() / 1e6))
    try:
        from sklearn.cluster import KMeans
        xh = base[0].reshape(-1, C)[fg[0].view(-1) != 0].cpu().numpy().astype("float64")
        c0 = res["km"]["centres"][0, :K_OBJ].cpu().numpy().astype("float64")
        t0 = time.perf_counter()
        KMeans(n_clusters=K_OBJ, init=c0, n_init=1, algorithm="lloyd", tol=0, max_iter=ITERS).fit(xh)
        one = (time.perf_counter() - t0) * 1e3
        lines.append("(e) sklearn KMeans on the host, one image %8.3f ms, x %d images = %8.1f ms (n_init=1; the reference asks for "
                     "n_init=35, max_iter=500)" % (one, B, one * B))
    except ImportError:
        lines.append("(e) sklearn does not import here: not measured")
    del m
    torch.cuda.empty_cache()
    if not opt.no_segment:
        seg = ReSeg(2, True, dtype=torch.bfloat16)
        seg.reset_parameters(seed=23)
        seg.eval()
        x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda")
        fmap = fg.view(B, -1).float()
        out = {}

        def attention():
            out["a"] = seg.segment(x, K_OBJ, sem_map=fmap)

        def embedding():
            out["e"] = seg.segment_embedding(x, sem_map=fmap, max_objects=K_OBJ, bandwidth=BW)

        t_a, t_e = alternate([attention, embedding], max(opt.calls // 2, 3), 2)
        lines.append("(d) whole inference, bf16 model, the same foreground map, at most %d objects: ReSeg.segment %8.3f ms   "
                     "ReSeg.segment_embedding (mean-shift) %8.3f ms" % (K_OBJ, t_a, t_e))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
