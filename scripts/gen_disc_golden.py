"""Generate tests/golden/disc.npz: the reference's own discriminative-loss functions on seeded embeddings, in float64.

Needs the reference tree (ISA_REFERENCE_ROOT, default as in oracle/ref_shim.py); its code/lib/losses/discriminative.py is
loaded by file path inside main(), so importing this script for cases() / case_inputs() never touches it:
    python scripts/gen_disc_golden.py
Per case (B, H, W, n_objects row, norm; C = 24, K = 32 planes, (delta_v, delta_d) = DELTAS[norm]) it stores float64 values of
    discriminative_loss (loss and means: unit means, var + 0.005 qreg)                      ref_loss, ref_means
    calculate_means(M='plain')                                                            means_plain
    calculate_variance_term on the unit and on the plain means                            var_unit, var_plain
    calculate_distance_term / calculate_regularization_term on the plain means            dist, reg
    calculate_q_regularization_term                                                       qreg
    full_loss = var_plain + dist + 0.001 reg
and autograd's gradient of ref_loss and of full_loss: every GRAD_STRIDE-th element and the float64 checksums (sum, sum of
squares, sum of magnitudes).  Every counted instance has a pixel and every image a counted foreground pixel (the reference
divides 0 by 0 otherwise); image 0 of the first shape also carries pixels on a plane past its n_objects (ignored by the
means and var, foreground for qreg).  The inputs are re-made from the seed by case_inputs, which the tests import.
The script also runs the reference in float32 on the same inputs and stores how far that is from float64, per case:
ref32_gap_loss (relative, the larger of the two forms) and ref32_gap_grad (relative L2, likewise) - the measure of what an
fp32 evaluation of these formulas can reach (tests/test_gpu_disc.py takes its bound from them)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

OUT = os.path.join(ROOT, "tests", "golden", "disc.npz")
C, K = 24, 32
DELTAS = {1: (11.5, 6.0), 2: (3.0, 1.5)}       # norm -> (delta_v, delta_d): about half of the hinges of either kind active
GRAD_STRIDE = 7
SHAPES = (((2, 24, 40), (3, 1)), ((3, 17, 23), (5, 2, 32)))


def cases():
    for (B, H, W), n_objects in SHAPES:
        for norm in (1, 2):
            yield B, H, W, n_objects, norm


def case_inputs(i):
    """Seeded embedding [B,C,H,W] float64, labels [B,H,W] int64 (0 background, k + 1 = plane k) and the n_objects row."""
    B, H, W, n_objects, _ = list(cases())[i]
    rs = np.random.RandomState(7100 + i)
    labels = np.zeros((B, H * W), dtype=np.int64)
    for b, nb in enumerate(n_objects):
        labels[b] = rs.randint(0, nb + 1, size=H * W)
        labels[b, rs.permutation(H * W)[:nb]] = np.arange(1, nb + 1)      # every counted instance has a pixel
    if n_objects == (3, 1):
        labels[0, 5:40:3] = 5                                             # a plane past n_objects[0]
        labels[0, :3] = (1, 2, 3)
    centres = rs.standard_normal((B, K + 1, C)) * 0.3
    x = rs.standard_normal((B, H * W, C)) * 0.6 + np.take_along_axis(centres, labels[:, :, None].repeat(C, 2), 1)
    x = x.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()
    return x, labels.reshape(B, H, W), n_objects


def planes_of(labels):
    """labels [B,H,W] -> disjoint planes [B,K,H,W] float64"""
    return (labels[:, None] == np.arange(1, K + 1)[None, :, None, None]).astype(np.float64)


def load_reference():
    sys.path[:0] = [os.path.join(ROOT, "oracle")]
    import ref_shim
    path = os.path.join(ref_shim.REF_ROOT, "code", "lib", "losses", "discriminative.py")
    spec = importlib.util.spec_from_file_location("reference_discriminative", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(D, x, labels, n_objects, norm, dtype):
    import torch
    n = [int(v) for v in n_objects]
    DELTA_V, DELTA_D = DELTAS[norm]
    tgt = torch.tensor(planes_of(labels), dtype=dtype)
    flat = lambda t: t.permute(0, 2, 3, 1).contiguous().view(t.shape[0], -1, t.shape[1])
    out = {}
    xr = torch.tensor(x, dtype=dtype, requires_grad=True)
    loss, means = D.discriminative_loss(xr, tgt, n, K, DELTA_V, DELTA_D, norm, False)
    loss.backward()
    out["ref_loss"], out["ref_means"], out["ref_grad"] = float(loss.detach()), means.detach().double().numpy(), xr.grad.double().numpy()
    xf = torch.tensor(x, dtype=dtype, requires_grad=True)
    inp, t = flat(xf), flat(tgt)
    plain = D.calculate_means(inp, t, n, K, False, M='plain')
    var = D.calculate_variance_term(inp, t, plain, n, DELTA_V, norm)
    dist = D.calculate_distance_term(plain, n, DELTA_D, norm, False)
    reg = D.calculate_regularization_term(plain, n, norm)
    full = var + dist + 0.001 * reg
    full.backward()
    out.update(means_plain=plain.detach().double().numpy(), var_plain=float(var.detach()), dist=float(dist.detach()),
               reg=float(reg.detach()), full_loss=float(full.detach()), full_grad=xf.grad.double().numpy())
    with torch.no_grad():
        xi = flat(torch.tensor(x, dtype=dtype))
        out["var_unit"] = float(D.calculate_variance_term(xi, t, means.detach(), n, DELTA_V, norm))
        out["qreg"] = float(D.calculate_q_regularization_term(xi, t))
    return out


def main():
    D = load_reference()
    import torch
    out = {}
    for i, (B, H, W, n_objects, norm) in enumerate(cases()):
        x, labels, _ = case_inputs(i)
        r64 = run_reference(D, x, labels, n_objects, norm, torch.float64)
        r32 = run_reference(D, x, labels, n_objects, norm, torch.float32)
        tag = "c%02d" % i
        out[tag + "/meta"] = np.array([B, H, W, norm] + list(n_objects), dtype=np.int64)
        for key in ("ref_loss", "full_loss", "var_unit", "var_plain", "dist", "reg", "qreg"):
            out[tag + "/" + key] = np.array(r64[key])
        out[tag + "/ref_means"], out[tag + "/means_plain"] = r64["ref_means"], r64["means_plain"]
        gaps_l, gaps_g = [], []
        for form in ("ref", "full"):
            g = r64[form + "_grad"].reshape(-1)
            out[tag + "/%s_grad_sub" % form] = g[::GRAD_STRIDE].copy()
            out[tag + "/%s_grad_sums" % form] = np.array([g.sum(), (g * g).sum(), np.abs(g).sum()])
            d = r32[form + "_grad"].reshape(-1) - g
            gaps_g.append(float(np.sqrt((d * d).sum() / (g * g).sum())))
            gaps_l.append(abs(r32[form + "_loss"] - r64[form + "_loss"]) / abs(r64[form + "_loss"]))
        out[tag + "/ref32_gap_loss"], out[tag + "/ref32_gap_grad"] = np.array(max(gaps_l)), np.array(max(gaps_g))
        print("case %d B=%d %dx%d n=%s norm=%d  ref %.6f full %.6f  fp32-vs-fp64: loss %.2e grad %.2e"
              % (i, B, H, W, n_objects, norm, r64["ref_loss"], r64["full_loss"], max(gaps_l), max(gaps_g)))
        try:
            import disc_np as R
            for form, unit in (("ref", "reference"), ("full", "full")):
                mine = R.form(unit, x, labels, n_objects, DELTAS[norm][0], DELTAS[norm][1], norm, K)
                g = r64[form + "_grad"]
                print("        restatement %-4s loss rel %.2e  grad rel L2 %.2e" % (
                    form, abs(mine["loss"] - r64[form + "_loss"]) / abs(r64[form + "_loss"]),
                    np.linalg.norm(mine["grad"] - g) / np.linalg.norm(g)))
        except ImportError:
            pass
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(list(cases())), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
