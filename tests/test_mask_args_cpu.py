"""The argument rules of the variance-mask entry points (csrc/mask_select.hip), without a device.

Every launcher validates before it touches the GPU, so on a machine without one a refused call returns VAM_EINVAL (-1)
with its message and an accepted call gets as far as the launch and returns VAM_EHIP (-2).  The pointers below are made-up
addresses: the module skips itself where a device is present, so that nothing can be launched on them.  Each bad row is
the entry's accepted row with one argument made bad; the refused rows also pin a key phrase of the rule that fires."""
import ctypes as C
import math

import pytest
import torch

from vampic import _lib as L

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only without a device")

EINVAL, EHIP = -1, -2
SIGMA, OUT, TABLE, MAP = 0x10000, 0x20000, 0x30000, 0x40000          # 16-byte aligned, never dereferenced on the host

# a window of 2 slices x 32 channels in buffers of 80 floats per pixel, 15 pixels, 2 images
SEG = dict(sigma=SIGMA, ld=80, batch_stride=15 * 80, slice_stride=32, n_batch=2, n_slice=2, n_pix=15, C=32)
DST = dict(out=OUT, ld_out=96, out_batch_stride=15 * 96, out_slice_stride=32)
SEG_NAMES = list(SEG)
DST_NAMES = list(DST)

ENTRIES = {
    "vam_variance_mask": (SEG_NAMES + ["pr"] + DST_NAMES + ["thr", "stream"], dict(pr=2.5)),
    "vam_variance_mask_levels": (SEG_NAMES + ["prs", "n_levels"] + DST_NAMES + ["level_stride", "thr", "stream"],
                                 dict(prs=[0.0, 0.5, 2.5, 12.0], n_levels=4, level_stride=2 * 15 * 96)),
    "vam_variance_layers": (SEG_NAMES + ["prs", "n_levels"] + DST_NAMES + ["thr", "stream"],
                            dict(prs=[0.0, 0.5, 2.5, 12.0], n_levels=4)),
    "vam_variance_layers_per_image": (SEG_NAMES + ["table"] + DST_NAMES + ["thr", "stream"], dict(table=TABLE)),
    "vam_variance_masks_per_image": (SEG_NAMES + ["table", "max_levels"] + DST_NAMES + ["level_stride", "thr", "stream"],
                                     dict(table=TABLE, max_levels=4, level_stride=2 * 15 * 96)),
    "vam_variance_mask_map": (SEG_NAMES + ["table", "level_map", "map_batch_stride"] + DST_NAMES + ["thr", "stream"],
                              dict(table=TABLE, level_map=MAP, map_batch_stride=1 << 20)),
}
LAYER_ENTRIES = ("vam_variance_layers", "vam_variance_layers_per_image")     # uint8 layer ids: 4-byte alignment


def _segment_rows(name):
    """(changed arguments, key phrase) of the rules that every launcher has."""
    rows = [({k: None}, "bad arguments") for k in ("sigma",)]
    rows += [({k: 0}, "bad arguments") for k in ("n_batch", "n_slice", "n_pix", "C")]
    rows += [({k: -1}, "bad arguments") for k in ("n_batch", "n_pix")]
    # the parent refused a missing layer array of vam_variance_layers in words of its own: the code alone is pinned
    rows += [({"out": None}, None if name == "vam_variance_layers" else "bad arguments")]
    rows += [({"C": 30}, "multiples of 4"), ({"ld": 82}, "multiples of 4"), ({"ld_out": 98}, "multiples of 4"),
             ({"batch_stride": 15 * 80 + 2}, "multiples of 4"), ({"slice_stride": 34}, "multiples of 4"),
             ({"out_batch_stride": 15 * 96 + 1}, "multiples of 4"), ({"out_slice_stride": 33}, "multiples of 4")]
    rows += [({"sigma": SIGMA + 4}, "alignment"), ({"sigma": SIGMA + 8}, "alignment")]
    rows += [({"out": OUT + 2}, "alignment")] if name in LAYER_ENTRIES else [({"out": OUT + 4}, "alignment"), ({"out": OUT + 8}, "alignment")]
    rows += [({"ld": 28}, "pixel stride"), ({"ld_out": 28}, "pixel stride")]
    rows += [({"n_pix": 500001}, "16M limit")]                               # 16 000 032 elements
    return rows


EXTRA = {
    "vam_variance_mask": [({"pr": -0.5}, "pr must be"), ({"pr": math.nan}, "pr must be")],
    "vam_variance_mask_levels": [({"level_stride": 2 * 15 * 96 + 2}, "multiples of 4"), ({"prs": None}, "levels, got"),
                                 ({"n_levels": 0}, "levels, got"), ({"prs": [0.5] * 9, "n_levels": 9}, "levels, got"),
                                 ({"prs": [0.5, -1.0, 2.0, 3.0]}, "pr must be"), ({"prs": [0.5, math.nan, 2.0, 3.0]}, "pr must be")],
    "vam_variance_layers": [({"prs": None}, "levels, got"), ({"n_levels": 0}, "levels, got"),
                            ({"prs": [0.5] * 33, "n_levels": 33}, "levels, got"),
                            ({"prs": [0.0, 2.5, 0.5, 12.0]}, "non-decreasing"), ({"prs": [-1.0, 0.5, 2.5, 12.0]}, "pr must be")],
    "vam_variance_layers_per_image": [({"table": None}, "bad arguments"), ({"table": TABLE + 2}, "alignment")],
    "vam_variance_masks_per_image": [({"table": None}, "bad arguments"), ({"table": TABLE + 2}, "alignment"),
                                     ({"max_levels": 0}, "levels, got"), ({"max_levels": 9}, "levels, got"),
                                     ({"level_stride": 2 * 15 * 96 + 2}, "multiples of 4")],
    "vam_variance_mask_map": [({"table": None}, "bad arguments"), ({"level_map": None}, "bad arguments"),
                              ({"table": TABLE + 2}, "alignment"), ({"map_batch_stride": 14}, "map_batch_stride")],
}
# lists that the wider kinds accept
ACCEPTED_MORE = {
    "vam_variance_mask": [{"pr": 0.0}, {"pr": 10.0}, {"pr": 1e9}, {"thr": OUT + 0x8000}, {"n_pix": 500000}],
    "vam_variance_mask_levels": [{"prs": [5.0, 0.0, 12.0, 0.5, 5.0, 1.0, 2.0, 3.0], "n_levels": 8}, {"prs": [2.5], "n_levels": 1}],
    "vam_variance_layers": [{"prs": [0.25 * i for i in range(32)], "n_levels": 32}, {"prs": [2.5, 2.5], "n_levels": 2},
                            {"out": OUT + 4}],
    "vam_variance_layers_per_image": [{"out": OUT + 4}, {"table": TABLE + 4}],
    "vam_variance_masks_per_image": [{"max_levels": 1}, {"max_levels": 8}],
    "vam_variance_mask_map": [{"map_batch_stride": 15}],
}

LAUNCH_ROWS = [(n, {}, EHIP, None) for n in ENTRIES]
LAUNCH_ROWS += [(n, ch, EHIP, None) for n, more in ACCEPTED_MORE.items() for ch in more]
LAUNCH_ROWS += [(n, ch, EINVAL, phrase) for n in ENTRIES for ch, phrase in _segment_rows(n) + EXTRA[n]]


def _id(row):
    name, changed, rc, _ = row
    what = ",".join(f"{k}={'list' if isinstance(v, list) else v}" for k, v in changed.items()) or "accepted"
    return f"{name[4:]}-{what}-{rc}"


def _call(name, changed):
    order, own = ENTRIES[name]
    args = dict(SEG, **DST, thr=None, stream=None, **own)
    args.update(changed)
    if isinstance(args.get("prs"), list):
        args["prs"] = (C.c_double * len(args["prs"]))(*args["prs"])
    lib = L.load()
    rc = getattr(lib, name)(*[args[k] for k in order])
    return rc, lib.vam_last_error().decode(errors="replace")


@pytest.mark.parametrize("row", LAUNCH_ROWS, ids=_id)
def test_launcher_argument_rules(row):
    name, changed, want, phrase = row
    rc, msg = _call(name, changed)
    assert rc == want, (rc, msg)
    if want == EHIP:
        assert "bad arguments" not in msg and "must be" not in msg, msg      # it got as far as the device
    elif phrase is not None:
        assert phrase in msg, msg


# ------------------------------------------------------------------------------------------------ the two host tables
PARAMS = {"vam_variance_layer_params": L.VAM_MAX_LAYER_LEVELS, "vam_variance_mask_params": L.VAM_MAX_MASK_LEVELS}
BASE_LISTS = [[0.0, 0.5, 2.5, 12.0], [1.25]]


def _params_rows(name):
    cap = PARAMS[name]
    rows = [({}, 0, None), ({"lists": [[0.5] * cap]}, 0, None), ({"lists": [[0.0], [10.0], [3.0]]}, 0, None), ({"n_pix": 500000}, 0, None)]
    rows += [({k: None}, EINVAL, "bad arguments") for k in ("prs", "n_levels", "table")]
    rows += [({k: 0}, EINVAL, "bad arguments") for k in ("n_batch", "levels_stride", "n_pix", "C")]
    rows += [({"n_pix": 500001}, EINVAL, "16M limit")]
    rows += [({"lists": [[1.0], []]}, EINVAL, "levels, got"), ({"lists": [[0.5] * (cap + 1)]}, EINVAL, "levels, got"),
             ({"counts": [5, 1]}, EINVAL, "levels, got")]                    # 5 levels in rows of levels_stride = 4
    rows += [({"lists": [[-1.0, 0.5]]}, EINVAL, "pr must be"), ({"lists": [[math.nan]]}, EINVAL, "pr must be")]
    if name == "vam_variance_layer_params":
        rows += [({"lists": [[0.0, 2.5, 0.5]]}, EINVAL, "non-decreasing")]
    else:
        rows += [({"lists": [[5.0, 0.0, 12.0, 0.5, 5.0]]}, 0, None)]       # any order, repeats allowed
    return rows


PARAMS_ROWS = [(n,) + r for n in PARAMS for r in _params_rows(n)]


@pytest.mark.parametrize("row", PARAMS_ROWS, ids=lambda r: f"{r[0][4:]}-{','.join(r[1]) or 'accepted'}-{r[2]}")
def test_params_argument_rules(row):
    name, changed, want, phrase = row
    lists = changed.get("lists", BASE_LISTS)
    width = max([len(r) for r in lists] + [1])
    counts = changed.get("counts", [len(r) for r in lists])
    flat = (C.c_double * (width * len(lists)))(*[v for r in lists for v in list(r) + [0.0] * (width - len(r))])
    nl = (C.c_int * len(lists))(*counts)
    table = (L.VamLayerParams * len(lists))()
    args = dict(prs=flat, n_levels=nl, n_batch=len(lists), levels_stride=width, n_pix=15, C=32, table=table)
    args.update({k: v for k, v in changed.items() if k not in ("lists", "counts")})
    lib = L.load()
    rc = getattr(lib, name)(*[args[k] for k in ("prs", "n_levels", "n_batch", "levels_stride", "n_pix", "C", "table")])
    msg = lib.vam_last_error().decode(errors="replace")
    assert rc == want, (rc, msg)
    if phrase is not None:
        assert phrase in msg, msg
