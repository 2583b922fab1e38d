"""The Viterbi decoder without a GPU: the numpy definition (tests/_viterbi_ref.py) against the recording of libcorrect's own answers
(tests/golden/viterbi_ref_io.npz, every frame on a fresh correct_convolutional), the coverage of the frame lengths the GPU tests
use, the module's surface, and what the library refuses before it looks for a device.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _viterbi_ref as V
from qdsp_amd import capi, fec, viterbi

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, ENODEV = -10001, -10004


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "viterbi_ref_io.npz"))


def test_definition_reproduces_the_recording(golden):
    """Byte for byte, the returned length included; frames of one code, kind and length are decoded as one batch."""
    cases, out, off = golden["cases"], golden["out"], golden["out_off"]
    assert len(cases) > 500
    seen = set()
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault(tuple(int(v) for v in c[:6]) + (int(c[7]),), []).append(i)
    for (rate, order, p0, p1, p2, soft, sets), idx in groups.items():
        poly = (p0, p1, p2)[:rate]
        x = np.stack([V.make_input(rate, order, poly, sets, bool(soft), int(cases[i][6]), int(cases[i][8])) for i in idx])
        y, _, _ = V.decode(rate, order, poly, x, sets, bool(soft))
        for k, i in enumerate(idx):
            rc = int(cases[i][9])
            assert rc == off[i + 1] - off[i] == V.frame_out_bytes(order, sets) == y.shape[1], (rate, order, soft, sets)
            assert y[k].tobytes() == out[off[i]:off[i + 1]].tobytes(), (rate, order, soft, int(cases[i][6]), sets)
        seen.add((rate, order, poly, soft))
    assert {(r, o, p, s) for (r, o), p in V.CODES.items() for s in (0, 1)} <= seen and len(seen) == 18
    assert {int(c[6]) for c in cases} == {V.KIND_CODED, V.KIND_NOISE, V.KIND_SATURATED}
    assert int(cases[:, 7].max()) == 8168


def test_encoder_matches_the_recorded_encodings(golden):
    codes, msgs, enc, off = golden["enc_codes"], golden["enc_msg"], golden["enc_out"], golden["enc_off"]
    assert len(codes) == 9
    for k, (rate, order, p0, p1, p2) in enumerate(codes.tolist()):
        e = V.encode(rate, order, (p0, p1, p2)[:rate], msgs[k])
        assert e.tobytes() == enc[off[k]:off[k + 1]].tobytes(), (rate, order)
        assert V.encode_bits(rate, order, (p0, p1, p2)[:rate], msgs[k]).size == rate * (8 * msgs.shape[1] + order + 1)


@pytest.mark.parametrize("rate,order", sorted(V.CODES))
def test_noiseless_round_trip(rate, order):
    poly = V.CODES[(rate, order)]
    rng = np.random.default_rng(order * 10 + rate)
    for nbytes in (1, 17, 40):
        msg = rng.integers(0, 256, (3, nbytes)).astype(np.uint8)
        sets = 8 * nbytes + order + 1
        bits = np.stack([V.encode_bits(rate, order, poly, m) for m in msg])
        hard, _, _ = V.decode(rate, order, poly, np.packbits(bits, axis=1), sets, False)
        soft, _, _ = V.decode(rate, order, poly, (255 * bits).astype(np.uint8), sets, True)
        assert hard.tobytes() == msg.tobytes() and soft.tobytes() == msg.tobytes()
        assert V.frame_out_bytes(order, sets) == nbytes


@pytest.mark.parametrize("rate,order", sorted(V.CODES))
def test_the_chosen_lengths_cover_every_path(rate, order):
    """edge_sets: frames without a traceback, the first traceback with the step before and after, the second, a traceback on the
    first, a middle and the last tail step, a renormalisation without a traceback, a bit count that is no multiple of 8 and
    is off the traceback boundary."""
    cap, g = 20 * order, 15 * order
    sch = {s: V.schedule(rate, order, s) for s in V.edge_sets(rate, order)}
    ntb = {s: sum(c in (V.TRACEBACK, V.BOTH) for c in sch[s][0]) for s in sch}
    assert min(sch) == order + 7 and sum(n == 0 for n in ntb.values()) >= 5
    first = cap + order - 1
    assert (ntb[first - 1], ntb[first], ntb[first + 1]) == (0, 1, 1) and sch[first][1] == [order - 1]
    assert (ntb[first + g - 1], ntb[first + g], ntb[first + g + 1]) == (1, 2, 2) and sch[first + g][1] == [order - 1]
    tails = sorted(k for s in sch for k in sch[s][1])
    assert tails[0] == 1 and tails[-1] == order - 1 and any(1 < k < order - 1 for k in tails)
    assert any(V.RENORM in c for c, _ in sch.values())
    assert any((s - order + 1) % 8 and (s - order + 1 - cap) % g and ntb[s] for s in sch)
    assert len(V.schedule(rate, order, order + 7)[0]) == 8


def test_a_renormalisation_and_a_traceback_fall_on_one_step():
    for sets in (1200, 1203):
        cases, _ = V.schedule(3, 7, sets)
        assert cases[1189] == V.BOTH and cases.count(V.BOTH) == 1
    assert V.renorm_interval(2) == 128 and V.renorm_interval(3) == 85
    x = np.stack([V.make_input(3, 7, V.CODES[(3, 7)], 1200, True, V.KIND_NOISE, 3)])
    _, cases, _ = V.decode(3, 7, V.CODES[(3, 7)], x, 1200, True)
    assert cases == V.schedule(3, 7, 1200)[0]


def test_module_surface():
    assert viterbi.__all__ == ["ViterbiDecoder", "Viterbi27"]
    assert set(fec.__all__) == {"RsDecoder", "FalconRs", "ccsds_dual_basis", "ccsds_randomizer"}
    for m in ("process", "process_batch", "process_ex", "last_kernel", "time_dev", "close"):
        assert callable(getattr(viterbi.ViterbiDecoder, m)), m
    assert issubclass(viterbi.Viterbi27, viterbi.ViterbiDecoder) and viterbi.Viterbi27.POLY == V.CODES[(2, 7)] == (0o161, 0o127)
    import qdsp_amd

    assert qdsp_amd.viterbi is viterbi
    for bad in ((4, 7, (1, 2, 3, 4), 100), (2, 5, (1, 2), 100), (2, 10, (1, 2), 100), (2, 7, (0o161, 0o327), 100), (2, 7, (0o161,), 100),
                (2, 7, (0o161, 0o127), 13), (2, 7, (0o161, 0o127), 65537)):
        with pytest.raises(ValueError):
            viterbi.ViterbiDecoder(*bad)
    names = set(capi.declared_symbols())
    assert {f"qdsp_hip_viterbi_{n}" for n in ("create", "frame_in_bytes", "frame_out_bytes", "process", "process_ex", "process_dev",
                                              "process_batch_dev", "destroy")} == {n for n in names if n.startswith("qdsp_hip_viterbi_")}


def test_create_refuses_what_is_out_of_its_domain():
    """Before the library looks for a device: with one, the in-domain calls succeed; without, they are QDSP_HIP_ENODEV."""
    L = capi.load()
    h = C.c_void_p()
    p27, p39 = (C.c_uint16 * 2)(0o161, 0o127), (C.c_uint16 * 3)(0o417, 0o627, 0o675)

    def create(rate, order, poly, sets, soft, nchan=1, maxb=4, hp=None):
        return L.qdsp_hip_viterbi_create(C.byref(h) if hp is None else hp, 0, nchan, maxb, rate, order, poly, sets, soft)

    for args in ((1, 7, p27, 100, 1), (4, 7, p27, 100, 1), (2, 5, p27, 100, 1), (2, 10, p27, 100, 1), (2, 7, None, 100, 1),
                 (2, 7, p27, 13, 1), (2, 7, p27, 0, 1), (2, 7, p27, -5, 1), (2, 7, p27, 65537, 1), (2, 7, p27, 100, 2), (2, 7, p27, 100, -1),
                 (2, 6, p27, 100, 1), (3, 8, p39, 100, 0), (2, 7, (C.c_uint16 * 2)(0o161, 128), 100, 1)):
        assert create(*args) == EINVAL and not h.value, args[:2] + args[3:]
    assert create(2, 7, p27, 100, 1, nchan=0) == EINVAL and create(2, 7, p27, 100, 1, maxb=(1 << 22) + 1) == EINVAL
    assert L.qdsp_hip_viterbi_create(None, 0, 1, 4, 2, 7, p27, 100, 1) == EINVAL
    n = C.c_int(0)
    has_gpu = L.qdsp_hip_device_count(C.byref(n)) == 0 and n.value > 0
    for args in ((2, 7, p27, 14, 1), (2, 7, p27, 65536, 0), (3, 9, p39, 16, 1), (3, 9, p39, 100, 0)):
        rc = create(*args)
        assert rc == (0 if has_gpu else ENODEV), args[:2] + args[3:]
        assert bool(h.value) == has_gpu
        if has_gpu:
            assert L.qdsp_hip_viterbi_frame_out_bytes(h) == (args[3] - args[1] + 1) // 8
            L.qdsp_hip_viterbi_destroy(h)
            assert L.qdsp_hip_viterbi_frame_out_bytes(h) == EINVAL
    # what is no live decoder is refused without being read
    junk = C.create_string_buffer(64)
    f = lambda name: getattr(L, "qdsp_hip_viterbi_" + name)  # noqa: E731
    for bad in (junk, None):
        assert f("frame_in_bytes")(bad) == EINVAL and f("frame_out_bytes")(bad) == EINVAL
        assert f("process")(bad, None, 0, None) == EINVAL and f("process_ex")(bad, None, 0, 0, None, 0) == EINVAL
        assert f("process_dev")(bad, None, 0, None, None) == EINVAL
        assert f("process_batch_dev")(bad, None, 0, 0, None, None, 0, None) == EINVAL
        assert f("destroy")(bad) is None
    assert L.qdsp_hip_rs_frame_in_bytes(junk) == EINVAL
