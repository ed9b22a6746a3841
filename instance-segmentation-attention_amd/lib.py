"""ctypes binding of libisa_kernels.so (include/isa_kernels.h).

There is deliberately NO fallback: if the HIP library is missing or a symbol is absent, importing
the product path raises.  The CPU oracle under oracle/ is never consulted from here.

Two handles onto the same symbols.  lib() is raw: every entry point returns its status (ABI tests, scripts).  checked() is
the product's: a non-zero status raises IsaError naming the symbol, so no call site wraps or checks.  On either handle a
data pointer (VP) takes a torch tensor as it is, so a call reads like its declaration in the header, stream last.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ISA_KERNELS_LIB: another build of the same library (A/B kernel timings inside one GPU session; scripts/kbench.py)
LIB_PATH = os.environ.get("ISA_KERNELS_LIB") or os.path.join(_HERE, "libisa_kernels.so")

F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_LEAKY, ACT_TANH = 0, 1, 2, 3, 4
IN_1X1, IN_3X3, IN_GATHER2 = 0, 1, 2
OUT_PLAIN, OUT_SHUFFLE2 = 0, 1
PLANES_U8_NHWK, PLANES_I64_NKHW, PLANES_F32_NKHW = 0, 1, 2
HIST_AGGREGATE, HIST_NAIVE = 0, 1
SEGSORT_TILE = 2048           # ISA_SEGSORT_TILE
CC_SPLIT, CC_LARGEST = 0, 1
CC_TILE_H, CC_TILE_W, CC_TAB_BYTES = 32, 64, 4608       # ISA_CC_TILE_H, ISA_CC_TILE_W, ISA_CC_TAB_BYTES


def segsort_table_elems(nseg, seglen):
    """ISA_SEGSORT_TABLE_ELEMS: uint32 elements of isa_segsort_kv_u32's table (digit table + chunk sums)."""
    tiles = (seglen + SEGSORT_TILE - 1) // SEGSORT_TILE
    return nseg * (256 * tiles + (tiles + 7) // 8)


def cc_label_scratch_bytes(n, h, w):
    """ISA_CC_LABEL_SCRATCH_BYTES: the union-find parents of isa_cc_label."""
    return n * h * w * 4


def cc_select_scratch_bytes(n, h, w):
    """ISA_CC_SELECT_SCRATCH_BYTES: areas by root pixel and the per-image tables of isa_cc_select."""
    return n * (h * w * 4 + CC_TAB_BYTES)


PROPS_ACC, PROPS_OUT, PROPS_MAX_SIDE = 16, 24, 32768      # ISA_PROPS_ACC, ISA_PROPS_OUT, ISA_PROPS_MAX_SIDE
ORDER_LABEL, ORDER_AREA, ORDER_RASTER = 0, 1, 2
CONTOUR_MAX_SIDE, CONTOUR_BLOCK, CONTOUR_COLS = 4096, 1024, 8     # ISA_CONTOUR_MAX_SIDE, ISA_CONTOUR_BLOCK, table columns


def contour_scratch_bytes(n, h, w):
    """ISA_CONTOUR_SCRATCH_BYTES: 48 bytes per possible edge (4 h w), 4 per lattice point and the block sums of the scans."""
    edges, points = 4 * h * w, ((h + 1) * (w + 1) + 3) // 4 * 4
    return n * (edges * 48 + points * 4 + (points // CONTOUR_BLOCK + 1) * 16 + (edges // CONTOUR_BLOCK + 1) * 16 + 16)


EDT_MAX_SIDE, EDT_COL_LANES, EDT_ROW_LANES = 4096, 64, 256    # ISA_EDT_MAX_SIDE, ISA_EDT_COL_LANES, ISA_EDT_ROW_LANES


def edt_scratch_bytes(n, h, w):
    """ISA_EDT_SCRATCH_BYTES: the two packed column entries per pixel of isa_edt2_u8."""
    return n * h * w * 8


ELASTIC_MAX_RADIUS, WARP_MAX_SIDE, WARP_MAX_CHANNELS = 64, 1024, 64      # ISA_ELASTIC_MAX_RADIUS, ISA_WARP_MAX_*
WARP_NEAREST, WARP_BILINEAR = 0, 1


def elastic_scratch_bytes(n, h, w):
    """ISA_ELASTIC_SCRATCH_BYTES: the row-blurred noise between the two passes of isa_elastic_field."""
    return n * h * w * 8


PASTE_MAX_SIDE, PASTE_MAX_PLANES = 4096, 32      # ISA_PASTE_MAX_SIDE, ISA_PASTE_MAX_PLANES


def copy_paste_scratch_bytes(n, k):
    """ISA_COPY_PASTE_SCRATCH_BYTES: the int32 area and remaining-area counters per image and plane of isa_copy_paste_u8."""
    return n * k * 8


DISC_MAX_K, DISC_CFG_FLOATS, DISC_CNT_STRIDE, ROW_CHUNKS = 32, 12, 36, 64     # ISA_DISC_*, ISA_ROW_CHUNKS


def disc_chunks(L):
    """ISA_DISC_CHUNKS: workgroups that share one image's pixels in the discriminative-loss passes."""
    return min((L + 1023) // 1024, ROW_CHUNKS)


CLUSTER_MAX_SHIFTS, CLUSTER_MAX_ITERS, CLUSTER_STATE_INTS, CLUSTER_CSLAB_STRIDE = 8, 64, 16, 36      # ISA_CLUSTER_*
CLUSTER_MAX_ROUNDS = 256


def cluster_scratch_bytes(n, L):
    """ISA_CLUSTER_SCRATCH_BYTES: slabs, loop state and moving centres of isa_cluster_meanshift / isa_cluster_kmeans."""
    return n * (8320 + disc_chunks(L) * 8488)


PHOTO_BRIGHTNESS, PHOTO_CONTRAST, PHOTO_SATURATION, PHOTO_HUE = 0, 1, 2, 3

_ERR = {-1: "ISA_EINVAL", -2: "ISA_EALIGN", -3: "ISA_EDTYPE", -4: "ISA_ELAUNCH", -5: "ISA_ENOMEM"}


class IsaTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c", C.c_int32), ("ld", C.c_int32), ("dtype", C.c_int32), ("groups", C.c_int32)]


class IsaBnFin(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p),
                ("invstd", C.c_void_p), ("count", C.c_float), ("momentum", C.c_float), ("eps", C.c_float),
                ("repeat", C.c_int32)]


class IsaPro(C.Structure):
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("bscale", C.c_void_p),
                ("act", C.c_int32), ("fin", C.POINTER(IsaBnFin))]


class IsaConvEp(C.Structure):
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("act", C.c_int32), ("res", C.c_void_p)]


class IsaBnBwd(C.Structure):
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("red", C.c_void_p), ("out_red", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("count", C.c_float), ("act", C.c_int32)]


class IsaBnUpd(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("count", C.c_float), ("c", C.c_int32)]


class IsaPackEntry(C.Structure):
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("kind", C.c_int32),
                ("n", C.c_int32), ("k", C.c_int32), ("taps", C.c_int32), ("kp", C.c_int32),
                ("kmap_off", C.c_int32), ("rows", C.c_int32)]


class IsaPhotoProg(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("op", C.c_uint8 * 4), ("factor", C.c_float * 4), ("hue_shift", C.c_uint8),
                ("use_lut", C.c_uint8), ("gray", C.c_uint8), ("chan", C.c_uint8 * 3), ("pad", C.c_uint8 * 2),
                ("lut", C.c_uint8 * 256)]


_plain = C.c_void_p.from_param          # looked up once: VP.from_param runs for every pointer argument of every launch


class VP(C.c_void_p):
    """A data pointer argument.  Takes what c_void_p takes (None, an int, a c_void_p, a ctypes array, byref(...)) and
    anything with a data_ptr(): a torch tensor passes as its device address, a view as the address of its first element."""

    @classmethod
    def from_param(cls, v):
        dp = getattr(v, "data_ptr", None)
        return _plain(v if dp is None else dp())


P_T, P_PRO, I32, F = C.POINTER(IsaTensor), C.POINTER(IsaPro), C.c_int32, C.c_float
I64 = C.c_int64
F64 = C.c_double
P_BN = C.POINTER(IsaBnBwd)

# name -> argtypes, exactly mirroring include/isa_kernels.h
SIGNATURES = {
    "isa_pack_weights": [VP, I32, VP, VP, VP, I32, VP],
    "isa_conv_gemm": [P_T, P_PRO, VP, I32, VP, P_T, I32, I32, VP, I32, VP],
    "isa_conv_gemm_ep": [P_T, P_PRO, VP, I32, VP, P_T, I32, VP, VP],
    "isa_dwpw_eval": [P_T, VP, VP, VP, VP, I32, VP, P_T, VP],
    "isa_conv_wgrad": [P_T, P_PRO, P_T, VP, VP, I32, I32, VP, I32, VP, I64, VP, VP],
    "isa_dwconv3x3": [P_T, P_PRO, VP, VP, P_T, VP, VP],
    "isa_dwconv3x3_dgrad": [P_T, VP, P_T, I32, VP],
    "isa_dwconv3x3_wgrad": [P_T, P_PRO, P_T, VP, VP, I32, VP, I64, VP, VP],
    "isa_dwconv3x3_bn_backward": [P_T, P_T, P_BN, P_T, P_PRO, P_BN, VP, VP, I32, P_T, I32, P_T, VP, I64, VP, VP],
    "isa_conv1x1_bn_backward": [P_T, P_T, P_BN, P_T, P_PRO, P_BN, VP, VP, P_T, I32, P_T, VP, I64, VP, VP],
    # the same two for convs with a bias: ... + dbias, and ... + bias, dbias
    "isa_dwconv3x3_bias_bn_backward": [P_T, P_T, P_BN, P_T, P_PRO, P_BN, VP, VP, I32, P_T, I32, P_T, VP, I64, VP, VP, VP],
    "isa_conv1x1_bias_bn_backward": [P_T, P_T, P_BN, P_T, P_PRO, P_BN, VP, VP, P_T, I32, P_T, VP, I64, VP, VP, VP, VP],
    "isa_slab_arena_create": [VP, I64, C.POINTER(C.c_void_p)],
    "isa_slab_arena_destroy": [VP],
    "isa_slab_arena_begin": [VP],
    "isa_slab_arena_flush": [VP, VP, VP, VP],
    "isa_bn_running_update": [C.POINTER(IsaBnUpd), I32, F, VP],
    "isa_d4_augment": [VP, VP, I32, I32, I32, I32, I32, VP, VP],
    "isa_rotate_nearest_u8": [VP, I32, I32, I32, I32, VP, I32, I32, VP, VP],
    "isa_rotate_bilinear_u8": [VP, I32, I32, I32, I32, VP, I32, I32, VP, VP, VP],
    "isa_cover_rows_u8": [VP, I32, I32, I32, I32, VP, VP, VP],
    "isa_plane_sums_u8": [VP, I32, I32, I32, I32, I32, I32, I32, I32, VP, VP],
    "isa_crop_planes_u8": [VP, I32, I32, I32, I32, I32, I32, VP, I32, I32, I32, VP, VP],
    "isa_resize_nearest_u8": [VP, I32, I32, I32, I32, VP, I32, I32, VP],
    "isa_resize_bilinear_u8": [VP, I32, I32, I32, I32, VP, I32, I32, VP, I64, VP],
    "isa_resize_lanczos_ws_bytes": [I32, I32, I32, I32, I32, I32, C.POINTER(C.c_int64)],
    "isa_resize_lanczos_u8": [VP, I32, I32, I32, I32, VP, I32, I32, VP, I64, VP],
    "isa_photometric_u8": [VP, VP, I32, I32, I32, VP, I32, VP, VP],
    "isa_collate_targets": [VP, VP, I32, I32, I32, I32, VP, VP, VP],
    "isa_collate_targets_k": [VP, VP, I32, I32, I32, I32, I32, VP, VP, VP, VP],
    "isa_bn_finalize": [VP, F, VP, VP, VP, VP, F, F, VP, VP, VP, VP, I32, I32, I32, VP],
    "isa_bn_bwd_reduce": [P_T, P_T, VP, VP, VP, VP, I32, VP, VP, VP],
    "isa_bn_bwd_apply": [P_T, P_T, VP, VP, VP, VP, I32, VP, VP, VP, F, I32, P_T, VP, VP, VP],
    "isa_affine_act_res": [P_T, P_PRO, P_T, P_T, VP, P_T, VP],
    "isa_axpy": [P_T, P_T, F, I32, VP],
    "isa_avgpool2": [P_T, P_T, VP],
    "isa_avgpool2_bwd": [P_T, P_T, I32, VP],
    "isa_avgpool3": [P_T, P_T, P_T, I32, VP],
    "isa_chan_mean": [P_T, P_PRO, VP, VP],
    "isa_se_fc": [VP, VP, VP, VP, VP, I32, I32, I32, VP, VP, VP],
    "isa_chan_argmax": [P_T, P_T, VP],
    "isa_mask_dot": [P_T, VP, VP, VP, VP, VP, VP],
    "isa_sp_softmax": [VP, VP, VP, VP, VP, VP, I32, I32, I64, VP, VP, VP, VP],
    "isa_scaled_stats": [P_T, VP, VP, VP],
    "isa_sp_apply": [P_T, VP, VP, VP, VP, P_T, VP],
    "isa_maskbn_stats": [P_T, VP, VP, VP, VP],
    "isa_maskbn_finalize": [VP, VP, I32, I32, VP, VP, VP, F, I32, VP],
    "isa_maskbn_apply_pool": [P_T, VP, VP, VP, VP, F, VP, VP],
    "isa_ins_softmax": [VP, VP, VP, I32, I32, I64, VP, VP, I32, VP, VP],
    "isa_row_argmax": [VP, VP, I32, I64, VP, VP],
    "isa_onehot_map": [VP, I32, I64, VP, VP],
    "isa_dropout_mask": [VP, I64, F, VP, VP],
    "isa_softmax_nchw": [P_T, VP, VP],
    "isa_pool_target": [VP, VP, VP, I32, I32, I32, I32, I32, VP, I32, VP],
    "isa_concat_aux": [P_T, VP, VP, I32, I32, I32, I32, VP],
    "isa_gate": [P_T, P_T, P_T, VP, VP],
    "isa_mask_loss_sums": [P_T, VP, VP, VP, VP],
    "isa_head_loss": [VP, VP, VP, I64, I32, VP, F, F, F, F, VP, I32, VP, VP, VP, I32, VP],
    "isa_sem_loss": [VP, I32, VP, VP, VP],
    "isa_mask_loss_grad": [P_T, VP, VP, VP, P_T, I32, VP],
    "isa_sem_loss_k_sums": [P_T, VP, VP, VP, VP],
    "isa_sem_loss_k_assemble": [VP, VP, I32, I32, VP, VP, VP],
    "isa_sem_loss_k_grad": [P_T, VP, VP, VP, P_T, I32, VP],
    "isa_sem_loss_k_sums_pw": [P_T, VP, VP, VP, VP, VP],
    "isa_sem_loss_k_grad_pw": [P_T, VP, VP, VP, VP, P_T, I32, VP],
    "isa_labels_from_onehot": [VP, I32, I32, I64, VP, VP, VP],
    # stable segmented radix sort and the Lovasz-Softmax criterion built on it
    "isa_segsort_kv_u32": [VP, VP, VP, VP, I32, I64, I32, I32, VP, VP, VP, I64, VP],
    "isa_lovasz_keys": [P_T, VP, I32, I32, I32, VP, VP, VP, VP],
    "isa_lovasz_coef": [VP, VP, VP, I32, I64, VP, VP, VP, VP],
    "isa_lovasz_assemble": [VP, VP, VP, I32, I32, I32, I64, VP, VP, VP, VP],
    "isa_lovasz_grad": [P_T, VP, VP, I32, P_T, I32, VP],
    # discriminative embedding loss (ReSeg.discriminative_loss, Trainer(disc_weight=...))
    "isa_disc_sums": [P_T, VP, I32, VP, VP, VP],
    "isa_disc_means": [VP, VP, VP, VP, I32, I64, VP, VP, VP, VP, VP],
    "isa_disc_hinge": [P_T, VP, I32, VP, VP, VP, I32, VP, VP, VP],
    "isa_disc_assemble": [VP, VP, VP, VP, VP, VP, VP, I32, I32, I64, VP, VP, VP, VP, VP],
    "isa_disc_grad": [P_T, VP, I32, VP, VP, VP, VP, VP, I32, P_T, I32, VP],
    # clustering the instance embedding (ReSeg.cluster_embedding, ReSeg.segment_embedding)
    "isa_cluster_meanshift": [P_T, VP, F, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, VP, VP],
    "isa_cluster_kmeans": [P_T, VP, VP, VP, I32, I32, VP, VP, VP, VP, VP, VP, VP],
    "isa_ins_softmax_bwd": [VP, VP, VP, VP, VP, I32, I32, I64, VP, I32, VP],
    "isa_maskbn_bwd": [P_T, VP, VP, VP, VP, F, VP, I32, VP, VP, VP, VP, P_T, I32, VP],
    "isa_sp_bwd": [P_T, P_T, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, F, I32, VP, P_T, I32,
                   VP, VP, VP, VP, VP, VP, VP, VP],
    "isa_gate_bwd": [P_T, P_T, VP, P_T, I32, VP, P_T, I32, VP],
    "isa_se_bwd": [P_T, P_T, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, VP, VP, P_T, I32, VP],
    "isa_scale_bc": [P_T, VP, P_T, I32, VP],
    "isa_sqnorm": [VP, I64, F, VP, VP],
    "isa_adadelta": [VP, VP, VP, VP, I64, F, F, F, F, VP, F, F, VP, VP],
    "isa_adam": [VP, VP, VP, VP, VP, VP, I64, F, F64, F64, F, F, VP, F, F, VP, VP],
    "isa_rmsprop": [VP, VP, VP, I64, F, F64, F, F, VP, F, F, VP, VP],
    "isa_sgd": [VP, VP, VP, I64, F, F64, F, VP, F, F, VP, VP],
    "isa_sdp_attention": [VP, VP, VP, VP, VP, VP, I32, I32, I64, I32, I32, F, I32, I32, I32, VP, I64, I32, VP],
    "isa_sdp_attention_bwd": [VP, VP, VP, VP, VP, VP, VP, VP, VP, I32, I32, I64, I32, I32, F, I32, I32, VP],
    "isa_sdp_scores": [VP, VP, VP, I32, I32, I32, I64, I32, I32, I32, VP],
    "isa_linear_ln": [VP, VP, VP, VP, VP, VP, F, I32, I32, I32, VP, VP],
    "isa_instance_norm_res": [P_T, P_T, P_T, F, VP, VP],
    "isa_local_attention": [P_T, P_T, P_T, VP, P_T, I32, F, VP],
    "isa_point_query": [VP, P_T, VP, VP],
    "isa_image_ex": [VP, P_T, VP],
    "isa_nchw_to_nhwc": [VP, I32, P_T, VP],
    "isa_nhwc_to_nchw": [P_T, VP, VP],
    # ground-truth-free instance inference (ReSeg.segment)
    "isa_seg_begin": [VP, VP, I32, I64, VP, VP, VP, VP, VP, VP, VP],
    "isa_seg_claim": [P_T, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP],
    # scoring instance predictions (ReSeg.score_instances)
    "isa_labels_from_planes": [VP, I32, I32, I32, I64, VP, VP],
    "isa_label_pair_hist": [VP, VP, I32, I64, I32, I32, VP, VP, I32, VP],
    "isa_instance_scores": [VP, I32, I32, I32, VP, VP, VP, VP],
    # scoring K-class semantic predictions (ReSeg.class_map, ReSeg.score_semantic)
    "isa_sem_confusion": [P_T, VP, I32, VP, VP, VP, VP],
    "isa_sem_scores": [VP, I32, I32, VP, VP],
    # connected components and instance clean-up (ReSeg.components, split_components, clean_instances)
    "isa_cc_label": [VP, I32, I32, I32, I32, VP, VP, VP, I64, VP],
    "isa_cc_select": [VP, VP, I32, I32, I32, I32, I32, I32, VP, VP, VP, VP, I64, VP],
    # measuring instances (ReSeg.instance_properties, select_instances)
    "isa_label_props": [VP, VP, I32, I32, I32, I32, I32, VP, VP, VP],
    "isa_instance_props": [VP, I32, I32, I32, I32, I32, VP, VP],
    "isa_props_select": [VP, I32, I32, I32, I32, I32, I32, I32, I32, I32, VP, VP, VP, VP],
    "isa_relabel_u8": [VP, VP, I32, I64, VP, VP],
    # tracing instance outlines (ReSeg.contours, instance_topology, polygons)
    "isa_contour_trace": [VP, I32, I32, I32, I32, I32, I32, VP, VP, VP, VP, I64, VP],
    "isa_contour_topology": [VP, VP, I32, I32, I32, VP, VP],
    # distance transform to the two nearest instances (ReSeg.distance_transform, border_weights, fill_instances)
    "isa_edt2_u8": [VP, I32, I32, I32, VP, VP, VP, VP, I64, VP],
    "isa_border_weights": [VP, VP, VP, VP, I32, I64, VP, VP],
    "isa_fill_labels": [VP, VP, VP, VP, I32, I32, I64, VP, VP, VP],
    # elastic deformation (data.elastic_field, data.warp, data.elastic; RecordLoader(elastic=True))
    "isa_elastic_field": [VP, VP, I32, I32, I32, VP, I32, VP, VP, I64, VP],
    "isa_warp_u8": [VP, VP, I32, I32, I32, I32, I32, VP, VP],
    # copy-paste augmentation (data.copy_paste; RecordLoader(copy_paste=True))
    "isa_copy_paste_u8": [VP, VP, VP, VP, VP, VP, I32, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, VP, I64, VP],
}


class IsaError(RuntimeError):
    pass


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "HIP kernel library not built: %s is missing. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C instance-segmentation-attention_amd/csrc`. There is no CPU fallback."
            % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: intended
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.isa_resize_bilinear_ws_bytes.argtypes = [I32] * 6       # the one entry point that returns a size, not a status
    lib.isa_resize_bilinear_ws_bytes.restype = C.c_int64
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def check(rc, what):
    if rc != 0:
        raise IsaError("%s failed: %s" % (what, _ERR.get(rc, rc)))


def _errcheck(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__)
    return rc


class _Checked:
    """The entry points of one loaded library as function objects of their own whose status is checked."""

    def __init__(self, raw):
        self.raw = raw
        for name, argtypes in SIGNATURES.items():
            fn = raw[name]                   # a fresh function object: raw.<name> keeps returning the status
            fn.argtypes, fn.restype, fn.errcheck = argtypes, C.c_int, _errcheck
            setattr(self, name, fn)
        self.isa_resize_bilinear_ws_bytes = raw.isa_resize_bilinear_ws_bytes      # a size, not a status


_checked = None


def checked():
    """The product's handle: lib()'s entry points, raising IsaError("<symbol> failed: <ISA_E...>") on a non-zero status."""
    global _checked
    raw = lib()
    if _checked is None or _checked.raw is not raw:
        _checked = _Checked(raw)
    return _checked


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16            # attention operators only
    raise IsaError("unsupported activation dtype %s" % dt)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def addr(t):
    """Device address of a torch tensor as a plain int (None -> NULL) for struct fields."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
