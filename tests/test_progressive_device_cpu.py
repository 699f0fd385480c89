"""The host side of the containers on the device coder: the threaded stream calls with ``lanes`` (the
interchange format of lane-split containers), the level grouping that bounds the layered encoder's scratch, the container
checks of ProgressiveDecoder, the status words of a layered launch and the new exports.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import vampic
from vampic import _lib as L
from vampic import bitstream as bs
from vampic import progressive as P
from test_rans_core_cpu import _stream_case, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LAYERS = 4


def _layer_jobs(t, seed=0):
    """Layer jobs as encode_batch builds them: one (symbols, indexes, layer ids) triple per stream, every selector a job.
    Selector 2 owns no element, some elements carry an id outside the range, one stream is shorter than 64 lanes."""
    rng = np.random.default_rng(seed)
    jobs = []
    for n in (512, 12, 333):
        sym, idx = _stream_case(t, n, seed=seed + n)
        layer = rng.choice(np.array([0, 1, 3, 7, 0xFF], dtype=np.uint8), size=n)
        jobs += [(sym, idx, layer, k) for k in range(N_LAYERS)]
    return jobs


@pytest.mark.parametrize("K", [2, 8, 64])
@pytest.mark.parametrize("threads", [None, 1, 3])
def test_stream_calls_with_lanes_equal_encode_lanes_and_round_trip(K, threads):
    t = _tables()
    jobs = _layer_jobs(t)
    got = bs.encode_streams(jobs, t, threads=threads, lanes=K)
    assert got == [bs.encode_lanes(s, i, t, K, ly, k) for s, i, ly, k in jobs]
    plain = [(s, i) for s, i, _, _ in jobs[::N_LAYERS]]                       # jobs without a layer array
    assert bs.encode_streams(plain, t, threads=threads, lanes=K) == [bs.encode_lanes(s, i, t, K) for s, i in plain]
    for j0 in range(0, len(jobs), N_LAYERS):                                  # the layers of one stream fill one array
        sym, idx, layer, _ = jobs[j0]
        out = np.full(sym.size, -7, dtype=np.int32)
        bs.decode_streams([(got[j0 + k], idx, out, layer, k) for k in range(N_LAYERS)], t, threads=threads, lanes=K)
        inside = layer < N_LAYERS
        assert np.array_equal(out[inside], sym[inside]) and (out[~inside] == -7).all()
    outs = [np.full(s.size, -7, dtype=np.int32) for s, _ in plain]
    bs.decode_streams([(b, i, o) for (s, i), b, o in zip(plain, bs.encode_streams(plain, t, lanes=K), outs)], t, lanes=K)
    assert all(np.array_equal(o, s) for (s, _), o in zip(plain, outs))


def test_one_lane_is_the_existing_call_byte_for_byte():
    t = _tables()
    jobs = _layer_jobs(t, seed=3)
    assert bs.encode_streams(jobs, t, lanes=1) == bs.encode_streams(jobs, t)
    assert bs.encode_streams(jobs, t) == [bs.encode_lanes(s, i, t, 1, ly, k) for s, i, ly, k in jobs]


def test_stream_calls_refuse_bad_lanes_and_name_the_failing_lane():
    t = _tables()
    sym, idx = _stream_case(t, 64, seed=1)
    for bad in (0, 3, 128, "8", None):
        with pytest.raises(ValueError, match="power of two"):
            bs.encode_streams([(sym, idx)], t, lanes=bad)
        with pytest.raises(ValueError, match="power of two"):
            bs.decode_streams([(b"", idx, np.zeros(64, np.int32))], t, lanes=bad)
    good = bs.encode_streams([(sym, idx)], t, lanes=8)[0]
    with pytest.raises(L.VamError, match="lane 0"):
        bs.decode_streams([(good[:28], idx, np.zeros(64, np.int32))], t, lanes=8)


@pytest.mark.parametrize("n_levels", [1, 2, 15, 32])
@pytest.mark.parametrize("level_bytes,budget", [(100, 1000), (100, 99), (100, 100), (100, 250), (7, 1 << 30), (41_984_000, None)])
def test_level_grouping_covers_all_levels_in_order_within_the_budget(n_levels, level_bytes, budget):
    groups = bs.layer_groups(n_levels, level_bytes, budget)
    assert groups[0][0] == 0 and groups[-1][1] == n_levels
    assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))              # consecutive, in order
    assert all(k1 > k0 for k0, k1 in groups)                                  # never empty
    limit = bs.LAYER_SCRATCH_BYTES if budget is None else budget
    for k0, k1 in groups:                                                     # within the budget, or a single level
        assert (k1 - k0) * level_bytes <= limit or k1 - k0 == 1
    if level_bytes <= limit:                                                  # and no more groups than the budget asks for
        per = limit // level_bytes
        assert len(groups) == -(-n_levels // per)


def test_level_grouping_defaults_and_refusals():
    assert bs.LAYER_SCRATCH_BYTES == 1 << 30
    # the 32 x 256 x 256 batch with the 15-level demo list: 320 streams per level, regions of 8 n + 64 bytes plus as much packed
    level_bytes = 2 * 320 * (8 * 8192 + 64)
    assert 0.62e9 < 15 * level_bytes < 0.64e9 and bs.layer_groups(15, level_bytes) == [(0, 15)]
    assert bs.layer_groups(15, level_bytes, 3 * level_bytes) == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15)]
    for bad in ((0, 10), (3, 0)):
        with pytest.raises(ValueError):
            bs.layer_groups(*bad)


def _container(shape=(1, 1), q_list=(0.5, 1), lanes=None):
    c = {"q_list": list(q_list), "shape": shape, "z": [b""], "base": [[b""]], "progressive": []}
    if lanes is not None:
        c["lanes"] = lanes
    return c


def test_check_containers_reads_the_lanes_key_and_refuses_mixed_batches():
    assert P.check_containers([_container(), _container()]) == ((1, 1), [0.5, 1.0], 1)
    assert P.check_containers([_container(lanes=8), _container(lanes=8)]) == ((1, 1), [0.5, 1.0], 8)
    assert P.check_containers([_container(lanes=1), _container()])[2] == 1    # no key is K = 1
    with pytest.raises(ValueError, match="same lanes"):
        P.check_containers([_container(lanes=8), _container()])
    with pytest.raises(ValueError, match="same lanes"):
        P.check_containers([_container(lanes=8), _container(lanes=64)])
    with pytest.raises(ValueError, match="power of two"):
        P.check_containers([_container(lanes=3)])
    with pytest.raises(ValueError, match="same shape and q_list"):
        P.check_containers([_container(), _container(shape=(1, 2))])
    with pytest.raises(ValueError, match="same shape and q_list"):
        P.check_containers([_container(), _container(q_list=(0.5, 2))])
    with pytest.raises(ValueError, match="no containers"):
        P.check_containers([])
    with pytest.raises(ValueError, match="non-decreasing"):
        P.check_containers([_container(q_list=(1, 0.5))])


def test_layer_status_words_name_image_level_slice_and_lane():
    B, ns = 2, 3
    st = np.zeros(4 * ns * B, dtype=np.int32)
    assert bs.layer_status_message(st, B, ns, "x") is None
    st[(2 * ns + 1) * B + 1] = 1                                              # level 2, slice 1, image 1
    assert bs.layer_status_message(st, B, ns, "x") == "x: stream (image 1, level 2, slice 1): bitstream truncated"
    assert "level 7, slice 1" in bs.layer_status_message(st, B, ns, "x", first_level=5)
    st[-1] = 2
    assert bs.layer_status_message(st, B, ns, "x").endswith("(2 streams failed)")
    st8 = np.zeros(ns * B * 8, dtype=np.int32)
    st8[((0 * ns + 2) * B + 0) * 8 + 5] = 6
    assert bs.layer_status_message(st8, B, ns, "x", lanes=8) == \
        "x: stream (image 0, level 0, slice 2), lane 5: bad stream (the header of 8 lane lengths does not match the string)"


def test_coder_argument_is_validated_before_any_gpu_use():
    import argparse
    import torch
    from conftest import README_ARGS
    net = vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu").eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        P.encode_batch(net, x, [0.5, 1], coder="gpu")
    with pytest.raises(ValueError, match="power of two"):
        P.encode_batch(net, x, [0.5, 1], lanes=3)
    net.coder = "gpu"
    with pytest.raises(ValueError, match="model.coder"):
        P.encode_batch(net, x, [0.5, 1])


def test_new_exports_are_in_the_library_and_the_header():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "vampic.h")).read()
    for name in ("vam_rans_layers_encode_device", "vam_rans_layers_decode_device"):
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"int vam_rans_pack_device\(const uint32_t\* regions, long cap_words, const int32_t\* lengths, int n_streams, "
                     r"uint32_t\* packed,\s+long packed_cap_words, int64_t\* offsets, void\* stream\);", header)   # unchanged
