"""Which test launches which side of every dtype / flag / width dispatch of the C entry points.

    python scripts/dispatch_coverage.py run tests -q        (writes dispatch_coverage.json, or $DISPATCH_COVERAGE_OUT)
    python scripts/dispatch_coverage.py table dispatch_coverage.json > profiles/launch_dispatch_coverage.txt

`run` wraps every ctypes function of lib.SIGNATURES and then runs the test runner in this process with the arguments
that follow; for each call that returned ISA_OK it records the calling test (the runner's PYTEST_CURRENT_TEST), the dtype
of the first tensor argument and the values the entry point's launch dispatches on (AX below restates those host-side
conditions).  Tests that start processes of their own are not followed.  `table` prints the table by source file."""
import collections, json, os, runpy, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = {}


def current_test():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" (")[0]


def S(a, cls):
    if a is None: return None
    if isinstance(a, cls): return a
    o = getattr(a, "_obj", None)
    if isinstance(o, cls): return o
    try:
        c = a.contents
        if isinstance(c, cls): return c
    except Exception:
        pass
    return None


def iv(a): return int(getattr(a, "value", a))
def nn(a):
    if a is None: return False
    v = getattr(a, "value", a)
    return v not in (None, 0)
def pow2(x): return x & (x - 1) == 0
def actc(a): return {2: "relu6", 0: "none"}.get(iv(a), "rt")


class Wrap:
    """callable stand-in for a ctypes function: attributes (argtypes, restype, ...) are the function's own"""
    def __init__(self, orig, call):
        object.__setattr__(self, "_o", orig); object.__setattr__(self, "_c", call)
    def __call__(self, *args): return self._c(*args)
    def __getattr__(self, k): return getattr(self._o, k)
    def __setattr__(self, k, v): setattr(self._o, k, v)


def install():
    sys.path[:0] = [ROOT]
    import isa_amd  # noqa
    from isa_amd import lib as L
    T = lambda a: S(a, L.IsaTensor)
    dtn = lambda code: {L.F32: "f32", L.BF16: "bf16"}.get(code, "dt%d" % code)
    w8 = lambda t: "w%d" % (min((t.c + 7) // 8, 4) * 8)

    def affine(a):
        pro = S(a[1], L.IsaPro)
        act = pro.act if pro else 0
        pi = bool(pro and pro.bscale) or nn(a[4])
        return ("none" if act == 0 else "rt", "pi" if pi else "nopi")

    def nchw(a):
        t = T(a[2]); cp = (t.c + 7) // 8 * 8
        rows = t.c <= 32 and t.ld == cp and (t.h * t.w) % 4 == 0 and t.ld % 8 == 0
        return (("rows" + w8(t)) if rows else "layout",)

    AX = {
        "isa_gate_bwd": lambda a: ("pow2" if pow2((T(a[1]).c + 7) // 8) else "npow2",),
        "isa_bn_bwd_reduce": lambda a: (actc(a[6]), "bscale" if nn(a[7]) else "nobscale"),
        "isa_bn_bwd_apply": lambda a: (actc(a[6]), "bscale" if nn(a[7]) else "nobscale"),
        "isa_affine_act_res": affine,
        "isa_axpy": lambda a: ("vec" if T(a[0]).c % 8 == 0 and T(a[0]).ld % 8 == 0 and T(a[1]).ld % 8 == 0 else "scalar",),
        "isa_avgpool3": lambda a: ("vec" if T(a[0]).c % 8 == 0 and T(a[0]).ld % 8 == 0 and T(a[2]).ld % 8 == 0 else "scalar",),
        "isa_nchw_to_nhwc": nchw,
        "isa_sdp_attention": lambda a: (dtn(iv(a[12])), "fast?" if iv(a[9]) == iv(a[10]) == 12 and nn(a[15]) and iv(a[13]) in (1, 2) else "general"),
        "isa_pack_weights": lambda a: (dtn(iv(a[5])),),
        "isa_disc_hinge": lambda a: ("norm%d" % iv(a[6]),),
        "isa_disc_assemble": lambda a: ("norm%d" % iv(a[7]),),
        "isa_disc_grad": lambda a: ("norm%d" % iv(a[8]),),
        "isa_seg_claim": lambda a: ("packed?" if T(a[0]).ld == 2 else "strided",),
    }
    for n in ("isa_lovasz_keys", "isa_lovasz_grad", "isa_sem_loss_k_sums", "isa_sem_loss_k_sums_pw", "isa_sem_loss_k_grad",
              "isa_sem_loss_k_grad_pw"):
        AX[n] = lambda a: (w8(T(a[0])),)

    lib = L.lib()
    for name in L.SIGNATURES:
        orig = getattr(lib, name)

        def call(*args, _orig=orig, _name=name):
            rc = _orig(*args)
            try:
                if rc == 0:
                    key = []
                    for a in args:
                        t = T(a)
                        if t is not None:
                            key.append(dtn(t.dtype)); break
                    if _name in AX: key += list(AX[_name](args))
                    k = _name + " " + " ".join(key)
                    cur = current_test()
                    r = REC.setdefault(k, [cur, 0, {}])
                    r[1] += 1
                    r[2].setdefault(cur.split("::")[0].replace("tests/", ""), cur.split("::")[-1])
            except Exception as e:  # never disturb a test
                REC.setdefault("ERR " + _name + " " + repr(e)[:80], [current_test(), 0, {}])[1] += 1
            return rc
        setattr(lib, name, Wrap(orig, call))


def run(args):
    install()
    sys.argv = ["pytest"] + args
    try:
        runpy.run_module("pytest", run_name="__main__")
    finally:
        with open(os.environ.get("DISPATCH_COVERAGE_OUT", "dispatch_coverage.json"), "w") as f:
            json.dump(REC, f, indent=0, sort_keys=True)


# ---- the table: converted entry points by source file
FILES = [
    ("attention.hip", "isa_mask_dot isa_scaled_stats isa_sp_apply isa_maskbn_stats isa_maskbn_apply_pool isa_softmax_nchw "
                      "isa_concat_aux isa_gate isa_mask_loss_sums"),
    ("head_bwd.hip", "isa_mask_loss_grad isa_maskbn_bwd isa_sp_bwd isa_gate_bwd isa_se_bwd isa_scale_bc"),
    ("elementwise.hip", "isa_pack_weights isa_bn_bwd_reduce isa_bn_bwd_apply isa_affine_act_res isa_axpy isa_avgpool2 "
                        "isa_avgpool2_bwd isa_avgpool3 isa_chan_mean isa_chan_argmax isa_nchw_to_nhwc isa_nhwc_to_nchw"),
    ("byname_attention.hip", "isa_sdp_attention isa_instance_norm_res isa_local_attention isa_point_query"),
    ("disc.hip", "isa_disc_sums isa_disc_hinge isa_disc_assemble isa_disc_grad"),
    ("cluster.hip", "isa_cluster_meanshift isa_cluster_kmeans"),
    ("lovasz.hip", "isa_lovasz_keys isa_lovasz_grad"),
    ("sem_loss.hip", "isa_sem_loss_k_sums isa_sem_loss_k_sums_pw isa_sem_loss_k_grad isa_sem_loss_k_grad_pw"),
    ("sem_score.hip", "isa_sem_confusion"),
    ("segment.hip", "isa_seg_claim"),
    ("image_ex.hip", "isa_image_ex"),
]


WHOLE = ("512_ddp", "1024", "entry", "model", "train", "poison", "ddp_rehearsal", "groups", "fused_dw", "criterion", "cluster")


def table(path):
    r = json.load(open(path))
    for k in sorted(r):
        if k.startswith("ERR"):
            print("!!", k, r[k])
    for f, names in FILES:
        print("\n%s" % f)
        for e in names.split():
            print("  %s" % e)
            keys = [k for k in sorted(r) if k.split()[0] == e]
            sides = collections.Counter(t for k in keys for t in r[k][2])
            for k in keys:
                side = " ".join(k.split()[1:]).replace("fast?", "head-width-12").replace("packed?", "ld2").replace("dt2", "f16")
                files = r[k][2]
                # name the operator's own test file: not a whole-network one, and the one that reaches most sides of this entry
                t = min(files, key=lambda t: (any(w in t for w in WHOLE), -sides[t], t))
                print("    %-28s %6d  %s::%s  (%d files)" % (side, r[k][1], t, files[t], len(files)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        table(sys.argv[2])
