"""The argument rules of the entropy-model and element-wise entry points (csrc/entropy.hip, csrc/elementwise.hip and the
element-wise launchers of csrc/train_gs.hip), without a device.

Every launcher validates before it touches the GPU, so on a machine without one a refused call returns VAM_EINVAL (-1)
with its message and an accepted call gets as far as the launch and returns VAM_EHIP (-2).  The device pointers below are
made-up addresses: the module skips itself where a device is present, so that nothing can be launched on them.  What an
entry reads on the host before it launches (``ks``, ``target3_host``, the ``vam_ew`` and ``vam_coder_tables`` structs) is real
host memory.  Each row is the entry's accepted call with one argument changed; a refused row also pins a key phrase of the
rule that fires.  The rows of a window are generated from what the entry demands of it: whether it may be absent, its
alignment (16 bytes for float / int32 vectors, 8 for the fp64 / int64 bins, 4 for uint8 layer ids, none for windows that
scalar loads read), and whether the pixel stride must cover C — a stride of C - 4 is recorded as accepted where the entry
does not ask."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

from vampic import _lib as L

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only without a device")

EINVAL, EHIP = -1, -2
CH, LD, NPIX, PPI = 32, 48, 30, 15                     # a window of 32 channels in rows of 48, 2 items of 15 pixels
LS = NPIX * LD                                         # level stride of the levels forms


def A(k):
    """the k-th made-up device address: 16-byte aligned, never dereferenced"""
    return 0x100000 * (k + 1)


# ptr / ld / ls: argument names (ls None: no level stride; ld None: a plain array).  words: (null, alignment, stride) phrases.
Win = namedtuple("Win", "ptr ld ls required align at_least_C")


def W(ptr, ld="ld_{}", ls=None, required=True, align=16, at_least_C=False):
    return Win(ptr, ld.format(ptr) if ld else None, ls.format(ptr) if ls else None, required, align, at_least_C)


def window_args(wins):
    """the accepted call's values of a list of windows"""
    out = {}
    for k, w in enumerate(wins):
        out[w.ptr] = A(k)
        if w.ld:
            out[w.ld] = LD
        if w.ls:
            out[w.ls] = LS
    return out


def window_rows(wins, words, C_name="C"):
    """(changed arguments, return code, phrase) of every rule of every window"""
    null, align, stride = words
    rows = []
    absent = {}
    for k, w in enumerate(wins):
        if w.required:
            rows.append(({w.ptr: None}, EINVAL, null))
        else:
            absent[w.ptr] = None
        if w.align == 16:
            rows += [({w.ptr: A(k) + 4}, EINVAL, align), ({w.ptr: A(k) + 8}, EINVAL, align)]
        elif w.align == 8:
            rows += [({w.ptr: A(k) + 4}, EINVAL, align), ({w.ptr: A(k) + 8}, EHIP, None)]
        elif w.align == 4:
            rows += [({w.ptr: A(k) + 2}, EINVAL, align), ({w.ptr: A(k) + 4}, EHIP, None)]
        else:
            rows += [({w.ptr: A(k) + 4}, EHIP, None)]
        if w.ld:
            rows.append(({w.ld: LD + 2}, EINVAL, stride) if w.align else ({w.ld: LD + 2}, EHIP, None))
            rows.append(({w.ld: CH - 4}, EINVAL, stride) if w.at_least_C else ({w.ld: CH - 4}, EHIP, None))
        if w.ls:
            rows.append(({w.ls: LS + 2}, EINVAL, stride))
    if absent:
        rows.append((absent, EHIP, None))
    return rows


ENTRIES = {}


def entry(key, order, wins, words, own=None, extra=(), build=None, skip=()):
    """key: the entry point, or entry/variant.  order: its C arguments by name.  own: the accepted values of what is not a
    window.  extra: rows of the other rules.  skip: generated rows an entry decides otherwise, restated in ``extra``."""
    base = dict(window_args(wins), stream=None, **(own or {}))
    rows = [({}, EHIP, None)] + [r for r in window_rows(wins, words) if tuple(r[0].items()) not in skip] + list(extra)
    ENTRIES[key] = dict(order=order, base=base, rows=rows, build=build)


RES = [W("y"), W("y2", required=False), W("mu"), W("sigma")]          # the residual window of the Gaussian entries
RES_C = [w._replace(at_least_C=True) for w in RES]
RES_ORDER = ["y", "ld_y", "y2", "ld_y2", "mu", "ld_mu", "sigma", "ld_sigma"]
EXTENT = [({"C": 30}, EINVAL), ({"C": 0}, EINVAL), ({"C": -4}, EINVAL), ({"n_pix": 0}, EINVAL), ({"n_pix": -1}, EINVAL)]


def extent(phrase, rows=EXTENT):
    return [(ch, rc, phrase) for ch, rc in rows]


def pl(*names):
    """argument names of windows: ptr, ld"""
    return [n for p in names for n in (p, "ld_" + p)]


def pll(*names):
    """argument names of level windows: ptr, ld, ls"""
    return [n for p in names for n in (p, "ld_" + p, "ls_" + p)]


def LV(ptr, required=True):
    return W(ptr, ls="ls_{}", required=required)


# ------------------------------------------------------------------------------------------------ the Gaussian tails
TAIL_WORDS = ("need y, mu, sigma", "16-byte alignment", "strides must be multiples of 4")
entry("vam_gauss_tail", RES_ORDER + pl("mask", "yhat", "lik", "sym") + ["log2sum", "pix_per_item", "n_pix", "C", "stream"],
      RES + [W(n, required=False) for n in ("mask", "yhat", "lik", "sym")], TAIL_WORDS,
      dict(log2sum=A(20), pix_per_item=PPI, n_pix=NPIX, C=CH),
      extent("C % 4 == 0") + [({"pix_per_item": 0}, EINVAL, "pix_per_item"), ({"log2sum": None, "pix_per_item": 0}, EHIP, None),
                                                   ({"log2sum": A(20) + 4}, EHIP, None), ({"pix_per_item": 7}, EHIP, None)])

entry("vam_gauss_levels_eval", RES_ORDER + pll("mask", "yhat", "lik", "sym") + ["log2sum", "pix_per_item", "n_levels", "n_pix", "C", "stream"],
      RES + [LV("mask")] + [LV(n, required=False) for n in ("yhat", "lik", "sym")], TAIL_WORDS,
      dict(log2sum=A(20), pix_per_item=PPI, n_levels=3, n_pix=NPIX, C=CH),
      extent("n_levels > 0 and C % 4 == 0") + [({"n_levels": 0}, EINVAL, "n_levels > 0"), ({"n_levels": 9}, EHIP, None), ({"n_levels": 40}, EHIP, None),
                                                ({"pix_per_item": 7}, EINVAL, "pix_per_item"), ({"pix_per_item": 0}, EINVAL, "pix_per_item"),
                                                ({"log2sum": None, "pix_per_item": 7}, EHIP, None),
                                                ({"n_pix": 1 << 31, "pix_per_item": 1, "n_levels": 1}, EINVAL, "too many items"),
                                                ({"n_pix": 1 << 30, "pix_per_item": 1, "n_levels": 2}, EINVAL, "too many items"),
                                                ({"n_pix": 1 << 30, "pix_per_item": 1, "n_levels": 1}, EHIP, None)],
      skip=((("mask", None),),))
ENTRIES["vam_gauss_levels_eval"]["rows"].append(({"mask": None}, EINVAL, "need y, mu, sigma, mask"))


def build_ks(args):
    ks = args["ks"]
    args["ks"] = None if ks is None else (C.c_int * len(ks))(*ks)


entry("vam_gauss_levels_decode", pl("sym", "layer", "mu") + ["ks", "n_levels", "yhat", "ld_yhat", "ls_yhat", "n_pix", "C", "stream"],
      [W("sym"), W("layer", align=4), W("mu"), LV("yhat")], ("bad arguments", "alignment", "strides must be multiples of 4"),
      dict(ks=[0, 1, 3, 255, 2, 7, 7, 0], n_levels=3, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"ks": None}, EINVAL, "bad arguments"), ({"n_levels": 0}, EINVAL, "levels, got"),
                                 ({"n_levels": L.VAM_MAX_MASK_LEVELS + 1}, EINVAL, "levels, got"), ({"n_levels": L.VAM_MAX_MASK_LEVELS}, EHIP, None),
                                 ({"n_levels": 1}, EHIP, None)],
      build=build_ks)

BINS = [W("layer", align=4, at_least_C=True), W("bits", ld=None, align=8), W("count", ld=None, align=8)]
LB_WORDS = ("must not be NULL", "alignment", "pixel strides must be multiples of 4 and >= C")
entry("vam_gauss_layer_bits", RES_ORDER + pl("layer") + ["n_levels", "bits", "count", "pix_per_item", "n_pix", "C", "stream"],
      RES_C + BINS, LB_WORDS, dict(n_levels=4, pix_per_item=PPI, n_pix=NPIX, C=CH),
      extent("need n_pix > 0 and C % 4 == 0") + [({"n_levels": 0}, EINVAL, "levels, got"), ({"n_levels": L.VAM_MAX_LAYER_LEVELS + 1}, EINVAL, "levels, got"),
                                                  ({"n_levels": L.VAM_MAX_LAYER_LEVELS}, EHIP, None), ({"n_levels": 1}, EHIP, None),
                                                  ({"pix_per_item": 7}, EINVAL, "pix_per_item must divide n_pix"), ({"pix_per_item": 0}, EINVAL, "pix_per_item must divide n_pix"),
                                                  ({"n_pix": 1 << 24, "pix_per_item": 1}, EINVAL, "item too large"), ({"n_pix": (1 << 24) - 1, "pix_per_item": 1}, EHIP, None),
                                                  ({"n_pix": 1 << 26, "pix_per_item": 1 << 26}, EINVAL, "item too large"),
                                                  ({"n_pix": 1 << 25, "pix_per_item": 1 << 25}, EHIP, None), ({"pix_per_item": NPIX}, EHIP, None)])

entry("vam_build_indexes", pl("sigma", "mask") + ["table", "n_table", "idx", "ld_idx", "n_pix", "C", "stream"],
      [W("sigma"), W("mask", required=False), W("idx")], ("bad arguments", "alignment", "alignment"),
      dict(table=A(20), n_table=64, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"table": None}, EINVAL, "bad arguments"), ({"table": A(20) + 4}, EHIP, None), ({"n_table": 1}, EINVAL, "table size"),
                                 ({"n_table": 257}, EINVAL, "table size"), ({"n_table": 2}, EHIP, None), ({"n_table": 256}, EHIP, None)])


# ------------------------------------------------------------------------------------------------ coded-size pricing
def build_tables(args):
    keep = args.pop("tables")
    t = L.VamCoderTables(args.pop("cost"), args.pop("sizes"), args.pop("offsets"), args.pop("n_cdfs"), args.pop("t_stride"))
    args["tables"] = C.byref(t) if keep else None


TABLES = dict(tables=True, cost=A(24), sizes=A(25), offsets=A(26), n_cdfs=64, t_stride=130)
CODED_OWN = dict(TABLES, n_levels=4, chans_per_stream=16, bits=A(21), count=A(22), pix_per_item=PPI, n_pix=NPIX, C=CH)


def coded_rows(no_tables="tables of stride"):
    """the rules the two coded-size entries share"""
    shared = "tables, bits and count must not be NULL"
    rows = [({k: None}, EINVAL, shared) for k in ("cost", "sizes", "offsets", "bits", "count")]
    rows += [({"n_cdfs": 0}, EINVAL, no_tables), ({"t_stride": 1}, EINVAL, "tables of stride"), ({"t_stride": 2}, EHIP, None)]
    rows += extent("need n_pix > 0 and C % 4 == 0")
    rows += [({"chans_per_stream": k}, EINVAL, "chans_per_stream") for k in (0, -4, 6, 24, 48, 64)]
    rows += [({"chans_per_stream": k}, EHIP, None) for k in (4, 8, 32)]
    rows += [({"n_levels": 0}, EINVAL, "levels, got"), ({"n_levels": L.VAM_MAX_LAYER_LEVELS + 1}, EINVAL, "levels, got"),
             ({"n_levels": L.VAM_MAX_LAYER_LEVELS}, EHIP, None), ({"n_levels": 1}, EHIP, None)]
    rows += [({"pix_per_item": 7}, EINVAL, "pix_per_item must divide n_pix"), ({"pix_per_item": 0}, EINVAL, "pix_per_item must divide n_pix")]
    # 2^20 streams: items x slices
    rows += [({"n_pix": 1 << 20, "pix_per_item": 1, "chans_per_stream": CH}, EINVAL, "item too large"),
             ({"n_pix": 1 << 19, "pix_per_item": 1, "chans_per_stream": 16}, EINVAL, "item too large"),
             ({"n_pix": (1 << 19) - 1, "pix_per_item": 1, "chans_per_stream": 16}, EHIP, None),
             ({"n_pix": 1 << 26, "pix_per_item": 1 << 26}, EINVAL, "item too large")]
    lay = "alignment / layer stride"
    rows += [({"layer": None}, EHIP, None), ({"layer": A(23) + 2}, EINVAL, lay), ({"layer": A(23) + 4}, EHIP, None), ({"ld_layer": LD + 2}, EINVAL, lay),
             ({"ld_layer": CH - 4}, EINVAL, lay), ({"layer": None, "ld_layer": 0}, EHIP, None), ({"bits": A(21) + 4}, EINVAL, lay),
             ({"count": A(22) + 4}, EINVAL, lay), ({"cost": A(24) + 4}, EINVAL, lay), ({"bits": A(21) + 8}, EHIP, None),
             ({"sizes": A(25) + 4}, EHIP, None)]
    return rows


entry("vam_coded_layer_bits", RES_ORDER + pl("layer") + ["n_levels", "scale_table", "n_table", "tables", "chans_per_stream", "bits", "count",
                                                         "pix_per_item", "n_pix", "C", "stream"],
      RES_C, ("must not be NULL", "16-byte alignment", "pixel strides must be multiples of 4 and >= C"),
      dict(CODED_OWN, layer=A(23), ld_layer=LD, scale_table=A(27), n_table=64),
      coded_rows("scale table of") + [({"scale_table": None}, EINVAL, "must not be NULL"), ({"scale_table": A(27) + 4}, EHIP, None),
                                            ({"n_table": 1}, EINVAL, "scale table of"), ({"n_table": 257}, EINVAL, "scale table of"),
                                            ({"n_table": 65}, EINVAL, "scale table of"), ({"n_table": 2}, EHIP, None),
                                            ({"tables": None}, EINVAL, "scale table of")],
      build=build_tables)

entry("vam_coded_symbol_bits", ["sym", "ld_sym", "idx", "ld_idx", "idx_base", "layer", "ld_layer", "n_levels", "tables", "chans_per_stream",
                                "bits", "count", "pix_per_item", "n_pix", "C", "stream"],
      [W("sym", at_least_C=True), W("idx", required=False, at_least_C=True)],
      ("sym must not be NULL", "16-byte alignment", "pixel strides must be multiples of 4 and >= C"),
      dict(CODED_OWN, layer=A(23), ld_layer=LD, idx_base=0),
      coded_rows() + [({"idx": None, "idx_base": 32}, EHIP, None), ({"idx": None, "idx_base": 33}, EINVAL, "must name tables"),
                                             ({"idx": None, "idx_base": -1}, EINVAL, "must name tables"), ({"idx_base": -1}, EHIP, None),
                                             ({"idx": None, "tables": None}, EINVAL, "must name tables"),
                                             ({"tables": None}, EINVAL, "tables, bits and count must not be NULL")],
      build=build_tables)


# ------------------------------------------------------------------------------------------------ the factorised prior
def SC(ptr, required=True, at_least_C=False):
    return W(ptr, required=required, align=0, at_least_C=at_least_C)


entry("vam_eb_forward_noise", ["z", "ld_z", "params", "C"] + pl("zhat", "lik", "sym") + ["log2sum", "pix_per_item", "n_pix", "noise", "ld_noise", "stream"],
      [SC("z"), SC("zhat", False), SC("lik", False), SC("sym", False)], ("bad arguments", None, None),
      dict(params=A(20), log2sum=A(21), pix_per_item=PPI, n_pix=NPIX, C=CH, noise=A(22), ld_noise=LD),
      extent("bad arguments", [r for r in EXTENT if r[0] != {"C": 30}]) +
      [({"C": 30}, EHIP, None), ({"C": 264, "ld_noise": 512}, EHIP, None), ({"C": 265, "ld_noise": 512}, EINVAL, "too large for LDS"), ({"C": 1025, "ld_noise": 2048}, EINVAL, "bad arguments"),
       ({"params": None}, EINVAL, "bad arguments"), ({"params": A(20) + 4}, EHIP, None), ({"pix_per_item": 0}, EINVAL, "pix_per_item"),
       ({"log2sum": None, "pix_per_item": 0}, EHIP, None), ({"noise": None}, EHIP, None), ({"noise": None, "ld_noise": 0}, EHIP, None),
       ({"noise": A(22) + 4}, EHIP, None), ({"ld_noise": LD + 2}, EHIP, None), ({"ld_noise": CH - 4}, EINVAL, "noise stride"),
       ({"ld_noise": CH}, EHIP, None)])


def build_target(args):
    t = args["target3_host"]
    args["target3_host"] = None if t is None else (C.c_float * 3)(*t)


entry("vam_eb_aux_loss", ["params", "C", "target3_host", "loss", "dquantiles", "stream"], [], (None, None, None),
      dict(params=A(0), C=CH, target3_host=[-6.9, 0.0, 6.9], loss=A(1), dquantiles=A(2)),
      [({k: None}, EINVAL, "bad arguments") for k in ("params", "target3_host", "loss", "dquantiles")] +
      [({"C": 0}, EINVAL, "bad arguments"), ({"C": -4}, EINVAL, "bad arguments"), ({"C": 30}, EHIP, None), ({"dquantiles": A(2) + 4}, EHIP, None)],
      build=build_target)

entry("vam_eb_train_bwd", ["z", "ld_z", "noise", "ld_noise", "params", "C", "grad_lik", "ld_grad_lik", "dz", "ld_dz", "dparams", "n_pix", "stream"],
      [SC(n, at_least_C=True) for n in ("z", "noise", "grad_lik", "dz")], ("bad arguments", None, "pixel strides"),
      dict(params=A(20), dparams=A(21), n_pix=NPIX, C=CH),
      extent("bad arguments", [r for r in EXTENT if r[0] != {"C": 30}]) +
      [({"C": 30}, EHIP, None), ({"params": None}, EINVAL, "bad arguments"), ({"dparams": None}, EINVAL, "bad arguments"), ({"params": A(20) + 4}, EHIP, None)])


# ------------------------------------------------------------------------------------------------ two-operand streams
def binary(name, a, b, out, align_words):
    entry(name, pl(a, b, out) + ["n_pix", "C", "stream"], [W(a), W(b), W(out)], ("bad arguments", align_words, "bad arguments"),
          dict(n_pix=NPIX, C=CH), extent("bad arguments"))


binary("vam_add", "a", "b", "out", "alignment")
binary("vam_mul", "a", "b", "out", "bad arguments")
binary("vam_leaky_bwd", "act", "dy", "dx", "bad arguments")
entry("vam_dequantize", pl("sym", "mu", "out") + ["n_pix", "C", "stream"], [W("sym"), W("mu", required=False), W("out")],
      ("bad arguments", "alignment", "bad arguments"), dict(n_pix=NPIX, C=CH), extent("bad arguments"))

# ------------------------------------------------------------------------------------------------ the training likelihood
TRAIN_ORDER = RES_ORDER + pl("mask", "noise", "grad_lik", "lik", "dmu", "dsigma") + ["n_pix", "C", "stream"]
TRAIN_WORDS = ("bad arguments", "alignment", "strides")
NEEDS = "forward needs lik, backward needs dmu and dsigma"
# forward: no grad_lik; the strides of dmu and dsigma are not looked at, their alignment is
entry("vam_gauss_train", TRAIN_ORDER, RES + [W("mask", required=False), W("noise"), W("lik")], TRAIN_WORDS,
      dict(grad_lik=None, ld_grad_lik=0, dmu=None, ld_dmu=0, dsigma=None, ld_dsigma=0, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"dmu": A(20), "ld_dmu": LD}, EHIP, None), ({"dmu": A(20) + 4, "ld_dmu": LD}, EINVAL, "alignment"),
                                 ({"dsigma": A(21) + 8, "ld_dsigma": LD}, EINVAL, "alignment"), ({"dmu": A(20), "ld_dmu": LD + 2}, EHIP, None),
                                 ({"dsigma": A(21), "ld_dsigma": LD + 2}, EHIP, None), ({"ld_grad_lik": 2}, EHIP, None)],
      skip=((("lik", None),),))
ENTRIES["vam_gauss_train"]["rows"].append(({"lik": None}, EINVAL, NEEDS))
# backward: grad_lik given; the stride of lik is not looked at, its alignment is
entry("vam_gauss_train/backward", TRAIN_ORDER, RES + [W("mask", required=False), W("noise"), W("grad_lik"), W("dmu"), W("dsigma")], TRAIN_WORDS,
      dict(lik=None, ld_lik=0, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"lik": A(20), "ld_lik": LD}, EHIP, None), ({"lik": A(20) + 4, "ld_lik": LD}, EINVAL, "alignment"),
                                 ({"lik": A(20), "ld_lik": LD + 2}, EHIP, None), ({"dmu": None}, EINVAL, NEEDS), ({"dsigma": None}, EINVAL, NEEDS),
                                 ({"grad_lik": None}, EINVAL, NEEDS)],                # without grad_lik it is a forward call without lik
      skip=((("dmu", None),), (("dsigma", None),), (("grad_lik", None),)))

entry("vam_gauss_levels_fwd", RES_ORDER + pll("mask", "noise", "rq", "lik") + ["n_levels", "n_pix", "C", "stream"],
      RES + [LV(n) for n in ("mask", "noise", "rq", "lik")], TRAIN_WORDS, dict(n_levels=3, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"n_levels": 0}, EINVAL, "bad arguments"), ({"n_levels": -1}, EINVAL, "bad arguments"), ({"n_levels": 40}, EHIP, None)])
entry("vam_gauss_levels_bwd", RES_ORDER + pll("mask", "noise", "grad_lik", "d_rq") + pl("gmu", "dsigma", "dy_top", "dy_sub") + ["n_levels", "n_pix", "C", "stream"],
      RES + [LV(n) for n in ("mask", "noise", "grad_lik", "d_rq")] + [W("gmu"), W("dsigma"), W("dy_top"), W("dy_sub", required=False)], TRAIN_WORDS,
      dict(n_levels=3, n_pix=NPIX, C=CH),
      extent("bad arguments") + [({"n_levels": 0}, EINVAL, "bad arguments"), ({"n_levels": -1}, EINVAL, "bad arguments"), ({"n_levels": 40}, EHIP, None)])


# ------------------------------------------------------------------------------------------------ vam_ew launchers
EW_WINS = ["in0", "in1", "in2", "in3", "out0", "out1", "out2"]


def fill_ew(e, args):
    for k, n in enumerate(EW_WINS):
        w = e.inp[k] if k < 4 else e.out[k - 4]
        w.ptr, w.ld = args.pop(n), args.pop("ld_" + n)
    e.n_pix, e.C, e.coef, e.flag = args.pop("n_pix"), args.pop("C"), 0.5, 0


def build_ew(args):
    e = L.VamEw()
    fill_ew(e, args)
    args["e"] = C.addressof(e) if args.pop("have_e") else None
    args["_keep"] = e


def ew_rows():
    rows = [({"have_e": False}, EINVAL, "bad arguments")] + extent("bad arguments")
    for k, n in enumerate(EW_WINS):
        which = f"input {k} alignment" if k < 4 else f"output {k - 4} alignment"
        rows += [({n: A(k) + 4}, EINVAL, which), ({n: A(k) + 8}, EINVAL, which), ({"ld_" + n: LD + 2}, EINVAL, which), ({"ld_" + n: CH - 4}, EHIP, None)]
    rows += [({n: None}, EINVAL, "op 4 needs 3 inputs") for n in ("in0", "in1", "in2")] + [({"in3": None}, EHIP, None)]
    rows += [({n: None}, EINVAL, "op 4 needs 3 outputs") for n in ("out0", "out1", "out2")]
    rows += [({"op": L.EW_AXPY, "in2": None, "in3": None, "out1": None, "out2": None}, EHIP, None),
             ({"op": L.EW_AXPY, "in1": None}, EINVAL, f"op {L.EW_AXPY} needs 2 inputs"), ({"op": 13}, EINVAL, "op 13"), ({"op": -1}, EINVAL, "op -1")]
    rows += [({"op": k}, EHIP, None) for k in range(13)]
    return rows


entry("vam_train_elementwise", ["op", "e", "stream"], [], (None, None, None),
      dict(window_args([W(n) for n in EW_WINS]), op=L.EW_GDN_BWD_PREP, have_e=True, n_pix=NPIX, C=CH), ew_rows(), build=build_ew)


def build_axpy(args):
    """n jobs: the changed arguments make the second one, the others are the accepted call's"""
    jobs = (L.VamEw * 9)()
    for j in range(9):
        fill_ew(jobs[j], dict(args if j == 1 else ENTRIES["vam_train_axpy_group"]["base"]))
    args["jobs"] = C.addressof(jobs) if args["jobs"] else None
    args["_keep"] = jobs


AXPY_WINS = [W("in0", at_least_C=True), W("in1", at_least_C=True), W("out0", at_least_C=True)]
entry("vam_train_axpy_group", ["jobs", "n", "stream"], AXPY_WINS, ("job 1 needs in0, in1, out0", "job 1 alignment", "job 1 row pitches"),
      dict(jobs=True, n=2, n_pix=NPIX, C=CH, **{k: v for n in ("in2", "in3", "out1", "out2") for k, v in ((n, None), ("ld_" + n, 0))}),
      extent("job 1 extent") + [({"jobs": False}, EINVAL, "jobs"), ({"n": 0}, EINVAL, "jobs"), ({"n": 9}, EINVAL, "1 .. 8 jobs"), ({"n": 8}, EHIP, None),
                                ({"n": 1, "C": 30}, EHIP, None)],                  # the bad job is the second one
      build=build_axpy)

# ------------------------------------------------------------------------------------------------ layouts of the backward
GRID = dict(B=2, H=3, W=5)
entry("vam_ps2_unshuffle", pl("src", "dst") + ["B", "H", "W", "Cq", "stream"], [SC("src"), SC("dst")], ("bad arguments", None, None),
      dict(GRID, Cq=8, ld_src=LD, ld_dst=LD),
      [({k: v}, EINVAL, "bad arguments") for k in ("B", "H", "W", "Cq") for v in (0, -1)] +
      [({"ld_src": 7}, EINVAL, "bad arguments"), ({"ld_src": 8}, EHIP, None), ({"ld_dst": 31}, EINVAL, "bad arguments"), ({"ld_dst": 32}, EHIP, None),
       ({"Cq": 7, "ld_src": 9}, EHIP, None)],
      skip=((("ld_src", CH - 4),), (("ld_dst", CH - 4),)))
entry("vam_upsample2_zero", pl("src", "dst") + ["B", "H", "W", "C", "stream"], [W("src", at_least_C=True), W("dst", at_least_C=True)],
      ("bad arguments", "alignment", "alignment"), dict(GRID, C=CH),
      [({k: v}, EINVAL, "bad arguments") for k in ("B", "H", "W", "C") for v in (0, -1)] + [({"C": 30}, EINVAL, "bad arguments")],
      skip=((("ld_src", CH - 4),), (("ld_dst", CH - 4),)))
ENTRIES["vam_upsample2_zero"]["rows"] += [({"ld_src": CH - 4}, EINVAL, "bad arguments"), ({"ld_dst": CH - 4}, EINVAL, "bad arguments"),
                                          ({"ld_src": CH}, EHIP, None)]

ROWS = [(key,) + row for key, e in ENTRIES.items() for row in e["rows"]]


def _id(row):
    key, changed, rc, _ = row
    what = ",".join(f"{k}={'list' if isinstance(v, list) else v}" for k, v in changed.items()) or "accepted"
    return f"{key[4:]}-{what}-{rc}"


def _call(key, changed):
    e = ENTRIES[key]
    args = dict(e["base"])
    args.update(changed)
    if e["build"]:
        e["build"](args)
    lib = L.load()
    rc = getattr(lib, key.split("/")[0])(*[args[k] for k in e["order"]])
    return rc, lib.vam_last_error().decode(errors="replace")


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_entry_argument_rules(row):
    key, changed, want, phrase = row
    rc, msg = _call(key, changed)
    assert rc == want, (rc, msg)
    if want == EHIP:
        assert msg.startswith("launch of"), msg                              # it got as far as the device
    elif phrase is not None:
        assert key.split("/")[0].replace("vam_eb_forward_noise", "vam_eb_forward") in msg and phrase in msg, msg


def test_every_entry_has_its_rows():
    """One accepted row, and at least one refused row, per entry; no row twice."""
    for key, e in ENTRIES.items():
        assert e["rows"][0] == ({}, EHIP, None), key
        assert any(rc == EINVAL for _, rc, _ in e["rows"]), key
        seen = [tuple(sorted((k, str(v)) for k, v in ch.items())) for ch, _, _ in e["rows"]]
        assert len(seen) == len(set(seen)), (key, [s for s in seen if seen.count(s) > 1])
