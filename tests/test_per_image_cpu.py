"""Per-image qualities without a GPU: the host arithmetic of the quality table of
vam_variance_masks_per_image (vam_variance_mask_params) against vam_variance_layer_params and against single-level records,
its refusals, and the argument validation of the model's per-image functions that precedes any GPU work."""
import ctypes as C

import numpy as np
import pytest
import torch

import vampic
from vampic import _lib as L, evaluate as EV, ops

FIELDS = ("k_lo", "k_hi", "w", "mode")


def _records(raw: np.ndarray):
    n = raw.size // C.sizeof(L.VamLayerParams)
    return [L.VamLayerParams.from_buffer_copy(raw[i * C.sizeof(L.VamLayerParams):(i + 1) * C.sizeof(L.VamLayerParams)].tobytes())
            for i in range(n)]


def _layer_table(lists, n_pix, ch):
    """vam_variance_layer_params' records for sorted lists (the existing per-image table)."""
    width = max(len(r) for r in lists)
    flat = (C.c_double * (width * len(lists)))(*[v for r in lists for v in list(r) + [0.0] * (width - len(r))])
    nl = (C.c_int * len(lists))(*[len(r) for r in lists])
    raw = np.zeros(len(lists) * C.sizeof(L.VamLayerParams), dtype=np.uint8)
    L.check(L.load().vam_variance_layer_params(flat, nl, len(lists), width, n_pix, ch, raw.ctypes.data), "vam_variance_layer_params")
    return _records(raw)


def _same(a, b, n):
    assert a.n_levels == b.n_levels == n and a.any_select == b.any_select
    for f in FIELDS:
        ga, gb = list(getattr(a, f)), list(getattr(b, f))
        if f == "w":                                  # bit patterns, not values
            ga, gb = np.array(ga, dtype=np.float32).view(np.uint32).tolist(), np.array(gb, dtype=np.float32).view(np.uint32).tolist()
        assert ga == gb, f


@pytest.mark.parametrize("n_pix,ch", [(256, 32), (1536, 32)])          # segments of 8192 and 49152 elements
def test_mask_params_equal_layer_params_on_sorted_lists(n_pix, ch):
    lists = [[0.0, 0.05, 0.5, 2.5, 9.99, 10.0, 12.0, 12.0], [1.25], [0.0, 0.0, 3.3]]
    got = _records(ops.mask_table(lists, n_pix, ch))
    want = _layer_table(lists, n_pix, ch)
    assert len(got) == len(want) == 3
    for g, w_, r in zip(got, want, lists):
        _same(g, w_, len(r))


@pytest.mark.parametrize("n_pix,ch", [(256, 32), (1536, 32)])
def test_mask_params_entry_by_entry_on_unsorted_and_repeated_lists(n_pix, ch):
    lists = [[5.0, 0.0, 12.0, 0.37, 5.0, 10.0, 0.001, 9.999], [10.0, 0.3], [7.7, 7.7, 0.0, 2.5, 0.05]]
    got = _records(ops.mask_table(lists, n_pix, ch))
    for rec, row in zip(got, lists):
        assert rec.n_levels == len(row)
        assert rec.any_select == int(any(0 < q < 10 for q in row))
        for lv, q in enumerate(row):
            one = _records(ops.mask_table([[q]], n_pix, ch))[0]
            ref = _layer_table([[q]], n_pix, ch)[0]
            for f in FIELDS:
                a, b, c_ = getattr(rec, f)[lv], getattr(one, f)[0], getattr(ref, f)[0]
                if f == "w":
                    a, b, c_ = (np.float32(v).view(np.uint32) for v in (a, b, c_))
                assert a == b == c_, (f, lv, q)
            assert rec.mode[lv] == (2 if q >= 10 else 1 if q == 0 else 0)
        for lv in range(len(row), L.VAM_MAX_LAYER_LEVELS):                # the rest of the record stays zero
            assert (rec.k_lo[lv], rec.k_hi[lv], rec.w[lv], rec.mode[lv]) == (0, 0, 0.0, 0)


def test_mask_params_refusals():
    with pytest.raises(L.VamError):
        ops.mask_table([[1.0], []], 256, 32)                              # no level
    with pytest.raises(L.VamError):
        ops.mask_table([[0.5] * (L.VAM_MAX_MASK_LEVELS + 1)], 256, 32)   # one too many
    assert _records(ops.mask_table([[0.5] * L.VAM_MAX_MASK_LEVELS], 256, 32))[0].n_levels == L.VAM_MAX_MASK_LEVELS
    with pytest.raises(L.VamError):
        ops.mask_table([[-1.0]], 256, 32)
    with pytest.raises(L.VamError):
        ops.mask_table([[float("nan")]], 256, 32)


def test_model_functions_validate_before_any_gpu_work(synth_model_cpu):
    net, _ = synth_model_cpu                  # a CPU model: anything that passed validation would fail at require_gpu or later
    x = torch.zeros(3, 3, 64, 64)
    for fn in (net.forward_per_image, net.compress_per_image):
        with pytest.raises(ValueError, match="one quality per image"):
            fn(x, [1.0, 2.0])
        with pytest.raises(ValueError, match=">= 0"):
            fn(x, [1.0, -0.5, 2.0])
        with pytest.raises(ValueError, match=">= 0"):
            fn(x, [1.0, float("nan"), 2.0])
    with pytest.raises(ValueError, match=r"forward_single_quality\(x\[zero\], 0\)"):
        net.forward_per_image(x, [1.0, 0.0, 2.0])
    with pytest.raises(ValueError, match="mixes"):
        net.forward_qualities_per_image(x, [[1.0, 2.0, 3.0], [0.0, 1.0, 0.0]])
    with pytest.raises(ValueError):
        net.forward_qualities_per_image(x, [[1.0, 2.0]])
    with pytest.raises(ValueError):
        net.forward_qualities_per_image(x, [[1.0, -2.0, 1.0]])
    with pytest.raises(ValueError, match="same shape"):
        net.decompress_per_image([{"strings": [[], []], "shape": (1, 1), "quality": 1.0},
                                  {"strings": [[], []], "shape": (1, 2), "quality": 1.0}])
    with pytest.raises(ValueError):
        net.decompress_per_image([{"strings": [[], []], "shape": (1, 1), "quality": -1.0}])
    with pytest.raises(ValueError):
        net.compress_to_bytes(x, [1000.0, 2000.0])
    with pytest.raises(ValueError):
        EV.rd_at_qualities(net, x, [[1.0, 2.0]])
