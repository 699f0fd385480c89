"""Pyramid viewports end to end on the GPU (``PyramidDecoder.viewport``, ``PyramidStream.viewport``, ``extract_viewport``, DESIGN
section 9zc) on the README model and the 150 x 200 picture of test_gpu_pyramid at 64 / 16: a viewport is the restatement
(tests/resample_ref.py) applied to the decode of its support window at its level, bit for bit, in fp32 and uint8, at a mark,
filled from the thumbnail at the cuts of test_gpu_pyramid_fill, through the receiver and from the server's extract.  Nothing
is asserted about PSNR values: the synthetic weights are untrained."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as RR                                          # noqa: E402
from test_gpu_embedded_schedule import _net                        # noqa: E402
from test_gpu_pyramid import H, SHAPES, W, _coded, _fresh          # noqa: E402
from test_gpu_pyramid_fill import _cuts                            # noqa: E402
from vampic import pyramid as PY                                  # noqa: E402

# (rect, out_hw, unit, the level it picks): the whole picture to 60 x 80; a rect across a blend band of level 0 to 64 x 64; a
# 3.3 x magnification at a third-of-a-pixel origin; a reduction by 2.7 that picks level 1; the whole picture from the thumbnail
VIEWS = [(None, (60, 80), 1, 1), ((40, 90, 70, 70), (64, 64), 1, 0), ((151, 182, 60, 60), (66, 66), 3, 0), ((7, 9, 130, 173), (48, 64), 1, 1),
         (None, (30, 40), 1, 2)]


def _same(got, want):
    got = got.cpu().numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _want(dec, rect, out_hw, unit, k, u8=False, **how):
    """The restatement on ``dec.decode`` of the support window at level k."""
    full = rect if rect is not None else (0, 0, H * unit, W * unit)
    win = PY.viewport_window(rect, out_hw, k, H, W, unit)
    assert win == RR.support_window(full, out_hw, k, H, W, unit)
    out = RR.resample(dec.decode(win, level=k, **how).cpu().numpy(), win, SHAPES[k], k, full, unit, out_hw)
    return RR.to_u8(out) if u8 else out


def test_the_whole_picture_at_half_size_is_level_one():
    dec = _fresh(_coded(), len(_coded()))
    assert PY.viewport_level(None, (75, 100), H, W, 3) == 1
    got = dec.viewport(None, (75, 100))
    assert got.dtype == torch.float32 and torch.equal(got, dec.decode(level=1)) and dec.last_chain[0][0] == 1
    assert torch.equal(dec.viewport(None, (75, 100), dtype=torch.uint8), dec.decode(level=1, dtype=torch.uint8))
    assert torch.equal(dec.viewport((0, 0, 150, 200), (150, 200)), dec.decode(level=0))


@pytest.mark.parametrize("rect,out_hw,unit,k", VIEWS)
def test_a_viewport_is_the_restatement_on_the_decode_of_its_support_window(rect, out_hw, unit, k):
    dec = _fresh(_coded(), len(_coded()))
    assert PY.viewport_level(rect, out_hw, H, W, 3, unit) == k
    got = dec.viewport(rect, out_hw, unit)
    assert tuple(got.shape) == (3,) + out_hw and _same(got, _want(dec, rect, out_hw, unit, k)) and dec.last_chain[0][0] == k
    assert _same(dec.viewport(rect, out_hw, unit, dtype=torch.uint8), _want(dec, rect, out_hw, unit, k, u8=True))
    at_mark = dec.viewport(rect, out_hw, unit, mark=1)
    assert _same(at_mark, _want(dec, rect, out_hw, unit, k, mark=1)) and not torch.equal(at_mark, got)
    assert _same(dec.viewport(rect, out_hw, unit, q=0.5, dtype=torch.uint8), _want(dec, rect, out_hw, unit, k, u8=True, q=0.5))


def test_an_explicit_level_at_a_scale_of_two_and_a_half():
    dec = _fresh(_coded(), len(_coded()))
    rect, out_hw = (10, 20, 100, 150), (40, 60)
    assert PY.viewport_level(rect, out_hw, H, W, 3) == 1
    got = dec.viewport(rect, out_hw, level=0)
    assert _same(got, _want(dec, rect, out_hw, 1, 0)) and dec.last_chain[0][0] == 0
    assert max(len(u) for _, u in PY.viewport_taps(rect, out_hw, 0, H, W)) in (5, 6)    # the loop path
    assert _same(dec.viewport(rect, out_hw, level=2), _want(dec, rect, out_hw, 1, 2))   # and a magnification of the thumbnail
    assert not torch.equal(got, dec.viewport(rect, out_hw))


@pytest.mark.parametrize("cut", ["need", "level 0: 5 heads"])
def test_a_filled_viewport_is_the_restatement_on_the_filled_decode(cut):
    n = _cuts()[cut]
    dec = PY.PyramidDecoder(_net(), _coded()[:n], group=4)
    for rect, out_hw, unit, k in VIEWS:
        got = dec.viewport(rect, out_hw, unit, fill=True)
        assert _same(got, _want(dec, rect, out_hw, unit, k, fill=True)), (rect, out_hw)
        assert dec.last_chain[0][0] == k and (cut != "need" or dec.last_chain[-1] == (2, [(0, 0)], [(0, 0)]))
        assert _same(dec.viewport(rect, out_hw, unit, fill=True, dtype=torch.uint8), _want(dec, rect, out_hw, unit, k, u8=True, fill=True))
    with pytest.raises(ValueError, match=r"PyramidDecoder.decode: level 1 does not decode: its bytes end before the heads of its tiles do" if cut == "need"
                       else r"PyramidDecoder.decode: level 0 does not decode"):
        dec.viewport(None, (60, 80)) if cut == "need" else dec.viewport(VIEWS[1][0], VIEWS[1][1])
    with pytest.raises(ValueError, match="PyramidDecoder.decode: q does not go with fill=True"):
        dec.viewport(None, (60, 80), q=0.5, fill=True)


def test_the_receiver_fed_unevenly_gives_the_fresh_decoder_s_viewports():
    data = _coded()
    st = PY.PyramidStream(_net(), group=5)
    with pytest.raises(ValueError, match="PyramidStream.viewport: nothing to decode yet: the header is not complete, 16 bytes are missing"):
        st.viewport(None, (60, 80))
    lay = PY.layout(data)
    at = 0
    for n in (lay["need_bytes"], _cuts()["level 0: 5 heads"], len(data)):
        for end in (at + 1, at + (n - at) // 3 + 1, n):                         # one byte, about a third, the rest
            st.feed(data[at:end])
            at = end
        dec = _fresh(data, n)
        for rect, out_hw, unit, k in VIEWS:
            for how in (dict(fill=True), dict(fill=True, dtype=torch.uint8)) + ((dict(),) if n == len(data) else ()):
                assert torch.equal(st.viewport(rect, out_hw, unit, **how), dec.viewport(rect, out_hw, unit, **how)), (n, rect, how)
                assert [e[0] for e in st.last_chain] == [e[0] for e in dec.last_chain]
    rect, out_hw, unit, k = VIEWS[1]
    st.viewport(rect, out_hw, unit)
    assert st.last_tiles and st.last_decoded == []                              # over cached tiles: no network
    pan = (rect[0] + 3, rect[1] - 5) + rect[2:]                                 # a pan step: one blend, one resample
    assert torch.equal(st.viewport(pan, out_hw, unit), _fresh(data, len(data)).viewport(pan, out_hw, unit)) and st.last_decoded == []
    assert torch.equal(st.viewport(pan, out_hw, unit, mark=1), _fresh(data, len(data)).viewport(pan, out_hw, unit, mark=1))
    with pytest.raises(ValueError, match="PyramidStream.viewport: level is 0 .. 2, got 3"):
        st.viewport(pan, out_hw, level=3)


@pytest.mark.parametrize("thumbnail", [True, False])
def test_the_server_s_extract_gives_the_full_stream_s_viewport(thumbnail):
    data = _coded()
    full = _fresh(data, len(data))
    for rect, out_hw, unit, k in VIEWS:
        ex = PY.extract_viewport(data, rect, out_hw, unit, thumbnail=thumbnail)
        assert len(ex) < len(data) and [lv["present"] for lv in PY.layout(ex)["levels"]] == [j == k or (thumbnail and j == 2) for j in range(3)]
        dec = PY.PyramidDecoder(_net(), ex, group=4)
        assert torch.equal(dec.viewport(rect, out_hw, unit, fill=thumbnail), full.viewport(rect, out_hw, unit)), (rect, out_hw)
        assert torch.equal(dec.viewport(rect, out_hw, unit, mark=1, dtype=torch.uint8, fill=thumbnail), full.viewport(rect, out_hw, unit, mark=1, dtype=torch.uint8))
        low = PY.extract_viewport(data, rect, out_hw, unit, rounds=2, thumbnail=thumbnail)    # cut in quality: mark 1 is whole
        assert len(low) < len(ex)
        assert torch.equal(PY.PyramidDecoder(_net(), low, group=4).viewport(rect, out_hw, unit, mark=1, fill=thumbnail), full.viewport(rect, out_hw, unit, mark=1))


def test_the_refusals():
    dec = _fresh(_coded(), len(_coded()))
    before = (list(dec.last_tiles), list(dec.last_chain))
    for kw, text in [(dict(rect=(0, 0, 151, 200)), r"the rect \(y0 0, x0 0, h 151, w 200\) / 1 does not lie inside the 150 x 200 picture"),
                     (dict(rect=(0, 0, 150, 601), unit=3), r"/ 3 does not lie inside the 150 x 200 picture"),
                     (dict(out_hw=(0, 80)), "out_hw is \\(rows, columns\\) of 1 .. 65536 each"), (dict(unit=0), "unit is 1 .. 256"),
                     (dict(level=3), "level is 0 .. 2, got 3"), (dict(level=-1), "level is 0 .. 2, got -1"), (dict(level=1.0), "level is an integer"),
                     (dict(dtype=torch.float16), "dtype is torch.float32 or torch.uint8"),
                     (dict(out_hw=(2, 2)), r"at level 2 has a scale of 18.75 x 25: above 16; level 3, of a pyramid of 4 levels, brings it to 16 or below"),
                     (dict(out_hw=(9, 12), level=0), r"at level 0 has a scale of 16.67 x 16.67: above 16; level 1, of a pyramid of 2 levels")]:
        args = {**dict(rect=None, out_hw=(60, 80)), **kw}
        with pytest.raises(ValueError, match=f"PyramidDecoder.viewport: .*{text}"):
            dec.viewport(**args)
    assert (list(dec.last_tiles), list(dec.last_chain)) == before               # refused before anything is decoded
    assert tuple(dec.viewport(None, (10, 13), level=0).shape) == (3, 10, 13)    # a scale of 15 and 15.4: allowed
