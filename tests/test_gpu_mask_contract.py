"""Every variance-mask entry point (csrc/mask_select.hip) against the numpy oracle directly: masks and layer ids byte for
byte, thresholds bit for bit.  All entries are instantiations of one kernel template, so none of them is the yardstick
of another here.  Shapes: B = 2 images x 2 slices of 32 channels at the latent sizes on either side of every dispatch
edge (4096 and 16384 float4 per segment), a partly filled wave, and one float4 (1x1, C = 4).  Sigma and the masks are
windows of wider buffers (ld != C) whose padding holds a sentinel that must come back unchanged."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic.synth as synth               # noqa: E402
import vampic_oracle as O                  # noqa: E402
from vampic import _lib as L, ops          # noqa: E402

B, NS = 2, 2
SENT = -7.0
# (h, w, C): float4 per segment = h * w * C / 4
SHAPES = [(5, 3, 32),       # 120: a partial wave, MAXV 4
          (16, 32, 32),     # 4096: the last size of MAXV 4
          (19, 27, 32),     # 4104: the first size of MAXV 16
          (32, 64, 32),     # 16384: the last size of MAXV 16
          (3, 683, 32),     # 16392: the first size of MAXV 0
          (1, 1, 4)]        # one float4
EIGHT = [0.0, 0.003, 0.5, 0.5, 2.5, 9.999, 10.0, 12.0]
THIRTY_TWO = sorted([0.0, 10.0, 0.003, 9.999] + [0.35 * i for i in range(1, 29)])
ONE = [2.5]
assert len(THIRTY_TWO) == L.VAM_MAX_LAYER_LEVELS and len(EIGHT) == L.VAM_MAX_MASK_LEVELS


class Case:
    """One shape: the seeded sigma with its planted values, on the device as a window, and the oracle's answers."""

    def __init__(self, h, w, C):
        self.h, self.w, self.C, self.hw, self.Ct = h, w, C, h * w, NS * C
        n = C * h * w
        s = synth.synth_sigma(B, NS * n, seed=11).reshape(B, NS * C, h, w).clone()
        seg = lambda b, j: s[b, j * C:(j + 1) * C]                    # noqa: E731  (a view)
        seg(0, 0)[:C // 2] = torch.round(seg(0, 0)[:C // 2] * 2) / 2   # a block of ties
        seg(1, 0).view(-1)[n // 3] = float("nan")                       # one segment with a NaN
        special = torch.tensor([0.0, -0.0, 1e-45, 1e-40, float("inf"), float("-inf")])[:min(6, n)]
        flat = seg(1, 1).reshape(-1)
        flat[torch.arange(special.numel()) * max(1, (n - 1) // 6)] = special
        seg(1, 1).copy_(flat.reshape(C, h, w))
        self.s = s.numpy()
        buf = torch.full((B, h, w, self.Ct + 16), 3.25)
        buf[..., 8:8 + self.Ct] = s.permute(0, 2, 3, 1)
        self.sigma = ops.View(buf.cuda(), 8, self.Ct)

    def seg(self, b, j):
        return self.s[b, j * self.C:(j + 1) * self.C]

    @functools.lru_cache(maxsize=None)
    def mask(self, b, j, q):
        """[C, h, w] float32 0/1"""
        return O.variance_mask_np(self.seg(b, j)[None], q)[0]

    @functools.lru_cache(maxsize=None)
    def thr(self, b, j, q):
        if q >= 10:
            return np.float32(-np.inf)
        if q == 0:
            return np.float32(np.inf)
        return np.float32(O.quantile_threshold_np(self.seg(b, j), q * 0.1))

    def masks(self, b, q):
        """[NS * C, h, w] of image b"""
        return np.concatenate([self.mask(b, j, q) for j in range(NS)])

    def layers(self, b, qs):
        """the first k with mask 1, else 255"""
        out = np.full((self.Ct, self.h, self.w), 255, dtype=np.uint8)
        for k in reversed(range(len(qs))):
            out[self.masks(b, qs[k]) == 1.0] = k
        return out

    def thr_rows(self, lists, rows):
        """[rows, B * NS]: level k of image b at [k, b * NS + j]; SENT beyond an image's list"""
        t = np.full((rows, B * NS), SENT, dtype=np.float32)
        for b, qs in enumerate(lists):
            for k, q in enumerate(qs):
                for j in range(NS):
                    t[k, b * NS + j] = self.thr(b, j, q)
        return t

    def mask_buffer(self, images):
        """A mask window with padding on both sides, everything at SENT."""
        return ops.View(torch.full((images, self.h, self.w, self.Ct + 8), SENT, device="cuda"), 4, self.Ct)

    def seg_args(self):
        sg = self.sigma
        return (sg.ptr, sg.ld, self.hw * sg.ld, self.C, B, NS, self.hw, self.C)


@functools.lru_cache(maxsize=None)
def case(shape):
    return Case(*shape)


def new_thr(rows):
    return torch.full((rows, B * NS), SENT, dtype=torch.float32, device="cuda")


def nchw(view):
    """the window as numpy [images, C, h, w], after checking that the padding around it kept its sentinel"""
    torch.cuda.synchronize()
    buf = view.buf.cpu()
    assert bool((buf[..., :view.c0] == SENT).all()) and bool((buf[..., view.c0 + view.C:] == SENT).all()), "padding overwritten"
    return buf[..., view.c0:view.c0 + view.C].permute(0, 3, 1, 2).contiguous().numpy()


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w_ = got.view(np.uint32 if got.dtype == np.float32 else np.uint8), want.view(np.uint32 if want.dtype == np.float32 else np.uint8)
    assert np.array_equal(g, w_), (what, int((g != w_).sum()))


def same_thr(got, want, what):
    """equal in bits; NaN where the oracle's is NaN"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, got, want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), (what, got, want)


def layer_buffer(c, images=B):
    """uint8 ids in a wider buffer (pixel stride Ct + 8, the window at 4), everything at 0xEE"""
    return torch.full((images, c.h, c.w, c.Ct + 8), 0xEE, dtype=torch.uint8, device="cuda")


def layer_ids(c, buf):
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[..., :4] == 0xEE).all()) and bool((host[..., 4 + c.Ct:] == 0xEE).all()), "padding overwritten"
    return host[..., 4:4 + c.Ct].permute(0, 3, 1, 2).contiguous().numpy()


def device_table(raw):
    return torch.from_numpy(raw).cuda()


# ------------------------------------------------------------------------------------------------ one quality
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_mask(shape):
    c = case(shape)
    for q in sorted(set(EIGHT)) + [1e9]:
        mask, thr = c.mask_buffer(B), new_thr(1)
        ops.variance_mask(c.sigma, q, mask, n_slice=NS, thr=thr)
        got = nchw(mask)
        for b in range(B):
            same_bytes(got[b], c.masks(b, q), ("mask", q, b))
        same_thr(thr, c.thr_rows([[q]] * B, 1), ("thr", q))
    # what the thresholds above were held to: +inf at quality 0, -inf from 10 on, NaN in the segment with the NaN
    assert c.thr(0, 0, 0.0) == np.inf and c.thr(0, 0, 12.0) == -np.inf and np.isnan(c.thr(1, 0, 2.5))


# ------------------------------------------------------------------------------------------------ one list
@pytest.mark.parametrize("qs", [EIGHT, ONE], ids=["eight", "one"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_mask_levels(shape, qs):
    c = case(shape)
    mask, thr = c.mask_buffer(len(qs) * B), new_thr(len(qs))
    ops.variance_mask_levels(c.sigma, qs, mask, n_slice=NS, thr=thr)
    got = nchw(mask)
    for k, q in enumerate(qs):
        for b in range(B):
            same_bytes(got[k * B + b], c.masks(b, q), ("mask", k, q, b))
    same_thr(thr, c.thr_rows([qs] * B, len(qs)), "thr")


@pytest.mark.parametrize("qs", [THIRTY_TWO, ONE], ids=["thirty-two", "one"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_layers(shape, qs):
    c = case(shape)
    buf, thr = layer_buffer(c), new_thr(len(qs))
    arr = (ctypes.c_double * len(qs))(*qs)
    ld = buf.shape[3]
    L.check(L.load().vam_variance_layers(*c.seg_args(), arr, len(qs), buf.data_ptr() + 4, ld, c.hw * ld, c.C, thr.data_ptr(),
                                         ops.stream_ptr()), "vam_variance_layers")
    got = layer_ids(c, buf)
    for b in range(B):
        same_bytes(got[b], c.layers(b, qs), ("layer", b))
    same_thr(thr, c.thr_rows([qs] * B, len(qs)), "thr")
    # the same through ops.variance_layers (a contiguous id array)
    ids = torch.full((B, c.h, c.w, c.Ct), 0xEE, dtype=torch.uint8, device="cuda")
    ops.variance_layers(c.sigma, qs, ids, n_slice=NS)
    torch.cuda.synchronize()
    same_bytes(ids.permute(0, 3, 1, 2).contiguous().cpu().numpy(), got, "ops.variance_layers")


# ------------------------------------------------------------------------------------------------ one list per image
PER_IMAGE_MASKS = [[EIGHT, [0.0]], [ONE, [12.0, 0.5, 0.003, 9.999, 0.5]]]
PER_IMAGE_LAYERS = [[THIRTY_TWO, [0.0]], [ONE, [0.5, 0.5, 7.0]]]


@pytest.mark.parametrize("lists", PER_IMAGE_MASKS, ids=["eight+zero", "one+five"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_masks_per_image(shape, lists):
    c = case(shape)
    NL = L.VAM_MAX_MASK_LEVELS
    mask, thr = c.mask_buffer(NL * B), new_thr(NL)
    table = device_table(ops.mask_table(lists, c.hw, c.C))
    ops.variance_masks_per_image(c.sigma, table, mask, n_slice=NS, thr=thr)
    got = nchw(mask)
    for b, qs in enumerate(lists):
        for k, q in enumerate(qs):
            same_bytes(got[k * B + b], c.masks(b, q), ("mask", b, k, q))
        assert bool((got[len(qs) * B + b::B] == SENT).all()), ("levels beyond the list", b)
    same_thr(thr, c.thr_rows(lists, NL), "thr")                        # rows beyond an image's list: untouched


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_masks_per_image_with_fewer_levels_than_a_record(shape):
    """max_levels smaller than a record's count writes nothing for that image; the other image is served."""
    c = case(shape)
    lists = [EIGHT, [0.0, 2.5]]
    mask, thr = c.mask_buffer(4 * B), new_thr(4)
    table = device_table(ops.mask_table(lists, c.hw, c.C))
    ops.variance_masks_per_image(c.sigma, table, mask, n_slice=NS, thr=thr, max_levels=4)
    got = nchw(mask)
    assert bool((got[0::B] == SENT).all())
    for k, q in enumerate(lists[1]):
        same_bytes(got[k * B + 1], c.masks(1, q), ("mask", k, q))
    assert bool((got[2 * B + 1::B] == SENT).all())
    same_thr(thr, c.thr_rows([[], lists[1]], 4), "thr")


@pytest.mark.parametrize("lists", PER_IMAGE_LAYERS, ids=["thirty-two+zero", "one+three"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_layers_per_image(shape, lists):
    c = case(shape)
    NL = L.VAM_MAX_LAYER_LEVELS
    buf, thr = layer_buffer(c), new_thr(NL)
    table = device_table(ops.layer_table(lists, c.hw, c.C))
    ld = buf.shape[3]
    L.check(L.load().vam_variance_layers_per_image(*c.seg_args(), table.data_ptr(), buf.data_ptr() + 4, ld, c.hw * ld, c.C,
                                                   thr.data_ptr(), ops.stream_ptr()), "vam_variance_layers_per_image")
    got = layer_ids(c, buf)
    for b, qs in enumerate(lists):
        same_bytes(got[b], c.layers(b, qs), ("layer", b))
    same_thr(thr, c.thr_rows(lists, NL), "thr")
    # the same through ops.variance_layers_per_image, which builds and copies the table itself
    ids = torch.full((B, c.h, c.w, c.Ct), 0xEE, dtype=torch.uint8, device="cuda")
    width = max(len(r) for r in lists)
    thr2 = new_thr(width)
    ops.variance_layers_per_image(c.sigma, lists, ids, n_slice=NS, thr=thr2)
    torch.cuda.synchronize()
    same_bytes(ids.permute(0, 3, 1, 2).contiguous().cpu().numpy(), got, "ops.variance_layers_per_image")
    same_thr(thr2, c.thr_rows(lists, width), "thr of ops.variance_layers_per_image")


# ------------------------------------------------------------------------------------------------ quality map
@pytest.mark.parametrize("lists", [[THIRTY_TWO, [0.0, 2.5, 10.0]], [ONE, [0.003]]], ids=["thirty-two+three", "one+one"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variance_mask_map(shape, lists):
    c = case(shape)
    NL = L.VAM_MAX_LAYER_LEVELS
    rng = np.random.default_rng(5)
    lm = np.stack([rng.integers(0, len(qs) + 3, size=c.hw) for qs in lists]).astype(np.uint8)    # some entries beyond the list
    lm[0, 0] = 255
    mask, thr = c.mask_buffer(B), new_thr(NL)
    table = device_table(ops.layer_table(lists, c.hw, c.C))
    ops.variance_mask_map(c.sigma, table, torch.from_numpy(lm).cuda(), mask, n_slice=NS, thr=thr)
    got = nchw(mask)
    for b, qs in enumerate(lists):
        want = np.zeros((c.Ct, c.hw), dtype=np.float32)                  # a map entry beyond the list writes 0
        for k, q in enumerate(qs):
            at = lm[b] == k
            want[:, at] = c.masks(b, q).reshape(c.Ct, c.hw)[:, at]
        same_bytes(got[b].reshape(c.Ct, c.hw), want, ("map", b))
    same_thr(thr, c.thr_rows(lists, NL), "thr")
