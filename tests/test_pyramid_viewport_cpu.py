"""Pyramid viewports on the host (vampic.pyramid.viewport_level / viewport_window / viewport_taps / extract_viewport, DESIGN
section 9zc) against the restatement of tests/resample_ref.py, which finds the taps by walking outwards from the centre: the
level, the support window and every tap of every row and column; the tap counts the kernel relies on; the tent the integer
weights stand for; a constant; the server's extract on the fabricated pyramids of test_pyramid_cpu; every refusal by its
message.  No model and no GPU are needed."""
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as RR
from test_pyramid_cpu import H, SHAPES, W, pyramid
from vampic import pyramid as PY, tiled as TL

PICTURES = [(1, 1), (5, 7), (38, 50), (150, 200)]
UNITS = [1, 3, 256]
SCALES = {"1": Fraction(1), "2": Fraction(2), "1.37": Fraction(137, 100), "1/3.3": Fraction(10, 33), "16": Fraction(16)}


def _fit(scale, N, k, unit, want):
    """(extent, out) along an axis of N level-0 pixels with ``extent / (out unit 2^k)`` = ``scale`` where that is a ratio of
    integers that fits, else the nearest extent; ``out`` is the largest one up to ``want`` that fits; None when none does."""
    for out in range(want, 0, -1):
        extent = scale * out * unit * 2 ** k
        extent = int(extent) if extent.denominator == 1 else max(1, round(extent))
        if extent <= N * unit:
            return extent, out
    return (N * unit, 1) if scale < 1 else None               # a magnification of the whole axis: the nearest there is


def _cases():
    """(name of the scale, H, W, k, unit, rect, out_hw): per picture, level, unit and scale every placement that fits: the
    origin 0, the far edge, and an odd origin inside; rows and columns take different outputs."""
    out = []
    for Hp, Wp in PICTURES:
        for k in range(3):
            for unit in UNITS:
                for name, s in SCALES.items():
                    fy, fx = _fit(s, Hp, k, unit, 13), _fit(s, Wp, k, unit, 17)
                    if fy is None or fx is None:
                        continue
                    (h, oh), (w, ow) = fy, fx
                    for y0, x0 in {(0, 0), (Hp * unit - h, Wp * unit - w), (min(1, Hp * unit - h), min(3, Wp * unit - w))}:
                        out.append((name, Hp, Wp, k, unit, (y0, x0, h, w), (oh, ow)))
    return out


CASES = _cases()


def test_the_cases_hold_every_picture_level_unit_and_scale():
    assert {c[0] for c in CASES} == set(SCALES) and {c[1:3] for c in CASES} == set(PICTURES)
    assert {c[3] for c in CASES} == {0, 1, 2} and {c[4] for c in CASES} == set(UNITS)
    for Hp, Wp in PICTURES:                                                     # and each picture meets each level and unit
        assert {(c[3], c[4]) for c in CASES if c[1:3] == (Hp, Wp)} == {(k, u) for k in range(3) for u in UNITS}
    exact = [c for c in CASES if c[0] == "16" and RR.scales(c[5], c[6], c[3], c[4]) == (16, 16)]
    assert len(exact) >= 20 and {c[3] for c in exact} == {0, 1, 2}


def test_taps_window_and_level_are_the_brute_force_s_over_all_rows_and_columns():
    for name, Hp, Wp, k, unit, rect, out_hw in CASES:
        Hk, Wk = RR.level_shape(Hp, Wp, k)
        sy, sx = RR.scales(rect, out_hw, k, unit)
        for axis, (origin, extent, o_n, s) in enumerate(((rect[0], rect[2], out_hw[0], sy), (rect[1], rect[3], out_hw[1], sx))):
            want = RR.axis_taps(origin, extent, o_n, k, unit)
            got = PY.viewport_taps(rect, out_hw, k, Hp, Wp, unit, axis)
            assert got == [(first, tuple(u)) for first, u in want], (name, Hp, Wp, k, unit, rect, out_hw, axis)
            D = 2 ** (k + 1) * o_n * unit
            for P, (first, u) in enumerate(want):
                assert all(v > 0 for v in u) and 1 <= len(u) <= 32              # a scale of at most 16
                if s <= 2:                                                      # the unrolled path: a - 1 .. a + 2
                    a = (2 * o_n * origin + (2 * P + 1) * extent - 2 ** k * o_n * unit) // D
                    assert len(u) <= 4 and a - 1 <= first and first + len(u) - 1 <= a + 2
        win = RR.support_window(rect, out_hw, k, Hp, Wp, unit)
        assert PY.viewport_window(rect, out_hw, k, Hp, Wp, unit) == win, (name, Hp, Wp, k, unit, rect, out_hw)
        assert 0 <= win[0] and 0 <= win[1] and win[2] >= 1 and win[3] >= 1 and win[0] + win[2] <= Hk and win[1] + win[3] <= Wk
        for n_levels in (1, 2, 3):
            if n_levels >= 2 and RR.level_shape(Hp, Wp, n_levels - 2) == (1, 1):
                continue                                                        # no such pyramid
            ks = RR.level(rect, out_hw, n_levels, unit)
            if max(RR.scales(rect, out_hw, ks, unit)) <= 16:
                assert PY.viewport_level(rect, out_hw, Hp, Wp, n_levels, unit) == ks
                lo, hi = sorted(RR.scales(rect, out_hw, ks, unit))
                assert ks == n_levels - 1 or (lo < 2) or ks == 0                # at k*: below 2 on an axis unless the levels ran out
                assert lo >= 1 or ks == 0
            else:
                with pytest.raises(ValueError, match="viewport_level: .*above 16; level"):
                    PY.viewport_level(rect, out_hw, Hp, Wp, n_levels, unit)


def test_just_above_sixteen_is_refused_and_the_message_names_the_level_that_would_do():
    seen = 0
    for name, Hp, Wp, k, unit, (y0, x0, h, w), out_hw in CASES:
        if name != "16" or RR.scales((y0, x0, h, w), out_hw, k, unit)[0] != 16 or y0 + h + 1 > Hp * unit:
            continue
        seen += 1
        over = (y0, x0, h + 1, w)
        assert len(PY.viewport_taps((y0, x0, h, w), out_hw, k, Hp, Wp, unit)[0][1]) in (31, 32)
        for fn in (lambda: PY.viewport_window(over, out_hw, k, Hp, Wp, unit), lambda: PY.viewport_taps(over, out_hw, k, Hp, Wp, unit, 0)):
            with pytest.raises(ValueError, match=rf"the rect \(h {h + 1}, w {w}\) / {unit} into {out_hw[0]} x {out_hw[1]} at level {k} has a scale of "
                                                 rf"16(\.\d+)? x 16: above 16; level {k + 1}, of a pyramid of {k + 2} levels, brings it to 16 or below"):
                fn()
    assert seen >= 5
    with pytest.raises(ValueError, match=r"viewport_level: .*at level 2 has a scale of 18.75 x 1: above 16; level 3, of a pyramid of 4 levels"):
        PY.viewport_level((0, 0, 150, 8), (2, 2), 150, 200, 3)                  # anisotropic: the columns stop the level at 2


def test_one_tap_of_weight_one_at_aligned_power_of_two_scales():
    for Hp, Wp, k, unit, rect, out_hw in [(150, 200, 1, 1, None, (75, 100)), (150, 200, 0, 1, None, (150, 200)),
                                          (150, 200, 2, 1, (0, 0, 148, 200), (37, 50)), (150, 200, 1, 3, (12, 24, 192, 192), (32, 32)),
                                          (38, 50, 0, 256, (256 * 5, 256 * 7, 256 * 20, 256 * 30), (20, 30)), (1, 1, 0, 1, None, (1, 1))]:
        full = rect if rect is not None else (0, 0, Hp * unit, Wp * unit)
        assert PY.viewport_level(rect, out_hw, Hp, Wp, 3 if Hp > 1 else 1, unit) == k
        for axis in (0, 1):
            taps = PY.viewport_taps(rect, out_hw, k, Hp, Wp, unit, axis)
            assert all(len(u) == 1 for _, u in taps)
            assert [first for first, _ in taps] == [(full[axis] >> k) // unit + P for P in range(out_hw[axis])]
            assert all(np.float32(u[0]) / np.float32(sum(u)) == np.float32(1.0) for _, u in taps)
        assert PY.viewport_window(rect, out_hw, k, Hp, Wp, unit) == ((full[0] >> k) // unit, (full[1] >> k) // unit) + tuple(out_hw)
        src = np.random.default_rng(k).random((2,) + RR.level_shape(Hp, Wp, k), dtype=np.float32)
        win = PY.viewport_window(rect, out_hw, k, Hp, Wp, unit)
        got = RR.resample(src, (0, 0) + src.shape[1:], src.shape[1:], k, full, unit, out_hw)
        assert np.array_equal(got, src[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])      # the source values come back


def test_the_integer_weights_are_the_normalised_tent():
    for name, Hp, Wp, k, unit, rect, out_hw in CASES[::3]:
        for axis in (0, 1):
            s = float(RR.scales(rect, out_hw, k, unit)[axis])
            o_n, half = out_hw[axis], max(1.0, s)
            D = 2 ** (k + 1) * o_n * unit
            for P, (first, u) in enumerate(PY.viewport_taps(rect, out_hw, k, Hp, Wp, unit, axis)):
                c = (2 * o_n * rect[axis] + (2 * P + 1) * rect[2 + axis] - 2 ** k * o_n * unit) / D
                lo = int(np.floor(c - half)) - 1
                tent = {i: max(0.0, 1.0 - abs(i - c) / half) for i in range(lo, lo + 2 * int(half) + 5)}
                total = sum(tent.values())
                want = {i: v / total for i, v in tent.items() if v > 1e-12}
                got = {first + j: v / sum(u) for j, v in enumerate(u) if v / sum(u) > 1e-12}
                assert got.keys() == want.keys() and all(abs(got[i] - want[i]) < 1e-12 for i in got), (name, rect, out_hw, k, unit, axis, P)


def test_a_constant_stays_within_the_bound_of_the_operations():
    """Every result is a sum of t_y t_x terms wy wx s; a term passes through three roundings per weight (two conversions, one
    division), one per multiply and at most t - 1 per sum on each axis: (t_y + t_x + 6) roundings of 2^-24 (see
    test_gpu_picture_resample's docstring), the weights adding up to 1."""
    for name, Hp, Wp, k, unit, rect, out_hw in CASES[::2]:
        Hk, Wk = RR.level_shape(Hp, Wp, k)
        for value in (np.float32(1) / np.float32(3), np.float32(-7.25)):
            src = np.full((1, Hk, Wk), value, dtype=np.float32)
            got = RR.resample(src, (0, 0, Hk, Wk), (Hk, Wk), k, rect, unit, out_hw)
            ty = max(len(u) for _, u in RR.axis_taps(rect[0], rect[2], out_hw[0], k, unit))
            tx = max(len(u) for _, u in RR.axis_taps(rect[1], rect[3], out_hw[1], k, unit))
            m = (ty + tx + 6) * 2.0 ** -24
            assert np.abs(got.astype(np.float64) - float(value)).max() <= m / (1 - m) * abs(float(value)), (name, rect, out_hw, k, unit)
            if ty == 1 and tx == 1:
                assert (got.view(np.uint32) == value.view(np.uint32)).all()


def test_the_restatement_is_the_float32_chain_written_out():
    rng = np.random.default_rng(5)
    src = (rng.random((2, 38, 50), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    rect, out_hw, k, unit = (7, 11, 139, 177), (61, 83), 2, 1                   # of a 150 x 200 picture: scales 0.57 and 0.53
    got = RR.resample(src, (0, 0, 38, 50), (38, 50), k, rect, unit, out_hw)
    ty, tx = RR.axis_taps(7, 139, 61, k, unit), RR.axis_taps(11, 177, 83, k, unit)
    f, cl = np.float32, lambda i, n: min(max(i, 0), n - 1)
    for c, Y, X in [(0, 0, 0), (1, 60, 82), (0, 30, 41), (1, 17, 3)]:
        acc = None
        for jr, uy in enumerate(ty[Y][1]):
            inner = None
            for jc, ux in enumerate(tx[X][1]):
                t = f(f(f(ux) / f(sum(tx[X][1]))) * src[c, cl(ty[Y][0] + jr, 38), cl(tx[X][0] + jc, 50)])
                inner = t if inner is None else f(inner + t)
            t = f(f(f(uy) / f(sum(ty[Y][1]))) * inner)
            acc = t if acc is None else f(acc + t)
        assert got[c, Y, X].view(np.uint32) == acc.view(np.uint32)
    exact, t_y, t_x = RR.resample_exact(src, (0, 0, 38, 50), (38, 50), k, rect, unit, out_hw)
    assert (t_y, t_x) == (2, 2) and np.abs(got - exact).max() <= 10 * 2.0 ** -24 * np.abs(src).max()
    win = RR.support_window(rect, out_hw, k, 150, 200, unit)                    # exactly the support window gives the same bits
    crop = src[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]]
    assert np.array_equal(RR.resample(crop, win, (38, 50), k, rect, unit, out_hw), got)


def test_extract_viewport_keeps_the_level_s_support_window_and_the_thumbnail():
    levels, data = pyramid()
    cases = [((40, 90, 60, 80), (30, 40), 1, 1), ((41, 93, 30, 17), (64, 64), 1, 0), ((3 * 40 + 1, 3 * 90 + 2, 3 * 50, 3 * 70), (23, 31), 3, 1),
             (None, (60, 80), 1, 1), (None, (30, 40), 1, 2), ((0, 0, 150, 200), (37, 50), 1, 2)]
    for rect, out_hw, unit, k in cases:
        assert PY.viewport_level(rect, out_hw, H, W, 3, unit) == k
        full = rect if rect is not None else (0, 0, H * unit, W * unit)
        win = RR.support_window(full, out_hw, k, H, W, unit)
        for rounds in (None, 2):
            ex = PY.extract_viewport(data, rect, out_hw, unit, rounds)
            lay = PY.layout(ex)
            assert len(ex) == lay["total"] and len(ex) < len(data)
            assert (lay["H"], lay["W"], lay["n_levels"]) == (H, W, 3) and [lv["present"] for lv in lay["levels"]] == [j in (k, 2) for j in range(3)]
            assert PY.level_stream(ex, 2) == TL.extract(levels[2], None, rounds)                # the thumbnail, whole
            if k != 2:
                assert PY.level_stream(ex, k) == TL.extract(levels[k], win, rounds)             # the support window's tiles
                y0, x0 = win[0] << k, win[1] << k
                win0 = (y0, x0, min(H, (win[0] + win[2]) << k) - y0, min(W, (win[1] + win[3]) << k) - x0)
                assert PY.window_at(win0, k, H, W) == win
                assert ex == PY.pack(H, W, [PY.level_stream(PY.extract(data, [j], win0 if j == k else None, rounds), j) if j in (k, 2) else None
                                            for j in range(3)])
            assert PY.extract_viewport(ex, rect, out_hw, unit, rounds) == ex == PY.extract_viewport(ex, rect, out_hw, unit)     # idempotent
            bare = PY.extract_viewport(data, rect, out_hw, unit, rounds, thumbnail=False)
            assert [lv["present"] for lv in PY.layout(bare)["levels"]] == [j == k for j in range(3)] and len(bare) <= len(ex)
            assert PY.level_stream(bare, k) == TL.extract(levels[k], win, rounds)
            assert PY.extract_viewport(bare, rect, out_hw, unit, thumbnail=False) == bare
    inner = PY.extract_viewport(data, (70, 70, 20, 20), (20, 20))               # level 0, one tile of twelve
    assert sum(map(sum, PY.layout(inner)["levels"][0]["layout"]["present"])) == 1
    with pytest.raises(ValueError, match="extract: level 1 is absent from this codestream; it holds the levels \\[0, 2\\]"):
        PY.extract_viewport(PY.extract(data, [0, 2]), (40, 90, 60, 80), (30, 40))
    with pytest.raises(ValueError, match=r"extract: level 1: extract: the window .* needs tile"):
        PY.extract_viewport(PY.extract_viewport(data, (0, 0, 60, 80), (30, 40)), (100, 120, 50, 80), (25, 40))
    with pytest.raises(ValueError, match="extract_viewport: thumbnail is True or False"):
        PY.extract_viewport(data, None, (30, 40), thumbnail=1)
    with pytest.raises(ValueError, match="extract_viewport: viewport_level: unit is 1 .. 256"):
        PY.extract_viewport(data, None, (30, 40), unit=0)
    with pytest.raises(ValueError, match=r"extract_viewport: viewport_level: .*at level 2 has a scale of 37.5 x 50: above 16; level 4, of a pyramid of 5"):
        PY.extract_viewport(data, None, (1, 1))


def test_every_refusal_names_what_is_wrong():
    ok = dict(rect=(0, 0, 150, 200), out_hw=(75, 100), k=1, H=150, W=200, unit=1)
    bad = [(dict(unit=0), "unit is 1 .. 256 .*got 0"), (dict(unit=257), "unit is 1 .. 256 .*got 257"), (dict(unit=1.0), "unit is an integer"),
           (dict(out_hw=(0, 5)), r"out_hw is \(rows, columns\) of 1 .. 65536 each, got \(0, 5\)"), (dict(out_hw=(5, 65537)), "of 1 .. 65536 each"),
           (dict(out_hw=(5,)), r"out_hw is \(rows, columns\), got \(5,\)"), (dict(out_hw=7), r"out_hw is \(rows, columns\), got 7"),
           (dict(out_hw=(5.0, 5)), "out_hw is an integer"), (dict(rect=(0, 0, 151, 200)), r"the rect \(y0 0, x0 0, h 151, w 200\) / 1 does not lie inside the 150 x 200 picture"),
           (dict(rect=(-1, 0, 10, 10)), "does not lie inside"), (dict(rect=(0, 0, 0, 10)), "does not lie inside"),
           (dict(rect=(0, 3 * 200 - 9, 10, 10), unit=3), r"the rect \(y0 0, x0 591, h 10, w 10\) / 3 does not lie inside the 150 x 200 picture"),
           (dict(rect=(0, 0, 10)), r"a rect is \(y0, x0, h, w\), got \(0, 0, 10\)"), (dict(rect=(0, 0, 10, 2.5)), "a rect entry is an integer"),
           (dict(H=0), "a picture of 0 x 200: sides are 1 .. "), (dict(W=(1 << 24) + 1), "a picture of 150 x 16777217"),
           (dict(k=-1), "level is 0 .. 15, got -1"), (dict(k=16), "level is 0 .. 15, got 16"), (dict(k=True), "level is an integer"),
           (dict(out_hw=(1, 1), k=0), r"has a scale of 150 x 200: above 16; level 4, of a pyramid of 5 levels, brings it to 16 or below")]
    for change, text in bad:
        a = {**ok, **change}
        for name, fn in (("viewport_window", lambda: PY.viewport_window(a["rect"], a["out_hw"], a["k"], a["H"], a["W"], a["unit"])),
                         ("viewport_taps", lambda: PY.viewport_taps(a["rect"], a["out_hw"], a["k"], a["H"], a["W"], a["unit"], 1))):
            with pytest.raises(ValueError, match=f"{name}: .*{text}"):
                fn()
        if "k" not in change:
            with pytest.raises(ValueError, match=f"viewport_level: .*{text}"):
                PY.viewport_level(a["rect"], a["out_hw"], a["H"], a["W"], 3, a["unit"])
    with pytest.raises(ValueError, match="viewport_taps: axis is 0 \\(rows\\) or 1 \\(columns\\), got 2"):
        PY.viewport_taps(None, (50, 50), 0, 150, 200, 1, 2)
    for n, text in ((0, "levels is 1 .. 16, got 0"), (17, "levels is 1 .. 16, got 17"), (10, "level 8 is 1 x 1 already"), (2.0, "n_levels is an integer")):
        with pytest.raises(ValueError, match=f"viewport_level: .*{text}"):
            PY.viewport_level(None, (5, 5), 150, 200, n)
    assert PY.viewport_level(None, (75, 100), 150, 200, 3) == 1 and PY.viewport_level(None, (75, 100), 150, 200, 1) == 0
    assert PY.viewport_level(None, (512, 768), 2048, 3072, 5) == 2 and PY.viewport_level((0, 0, 100, 100), (330, 330), 150, 200, 3) == 0
    assert PY.viewport_window(None, (75, 100), 1, 150, 200) == (0, 0, 75, 100) == PY.viewport_window((0, 0, 150, 200), (75, 100), 1, 150, 200)
    assert SHAPES[1] == (75, 100)
