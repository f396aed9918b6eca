"""The message batch's Poly1305 decomposition (suruga_amd/csrc/sg_msg_batch.hip)
restated in Python integers from the exported plan (sg_msg_batch_plan_for) and
compared with the oracle's sequential Poly1305 (poly1305.rs:195-312) on each
message's MAC stream, and the properties of that plan.  CPU only."""
from __future__ import annotations

import pytest

import msg_batch_support as mb
from mac_forge import mac_stream
from msg_batch_support import rnd


@pytest.fixture(scope="module", autouse=True)
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def plan_of(shapes, groups):
    from suruga_amd import msg

    return msg.batch_plan_for([n for _, n in shapes], [a for a, _ in shapes], groups)


@pytest.fixture(scope="module")
def edge_streams(oracle):
    shapes = mb.edge_shapes()
    data = rnd("batch stream", max(a + n for a, n in shapes))
    streams = [mac_stream(data[:a], data[a:a + n]) for a, n in shapes]
    rs = [(rnd(f"batch r{i}", 16), rnd(f"batch s{i}", 16)) for i in range(len(shapes))]
    want = [oracle.poly1305(st, r16, s16) for st, (r16, s16) in zip(streams, rs)]  # once, shared
    return shapes, streams, rs, want


def test_edge_batch_is_thirteen_messages_of_thirty_tiles():
    from suruga_amd import msg

    shapes = mb.edge_shapes()
    assert msg.plan_for(0, 0)["tile_bytes"] == mb.TB
    assert len(shapes) == 13 and sum(mb.tiles_of(a, n) for a, n in shapes) == 30
    assert plan_of(shapes, 0)["tiles"] == 30


@pytest.mark.parametrize("groups", mb.GROUPS)
def test_batch_decomposition_equals_the_sequential_mac(edge_streams, groups):
    shapes, streams, rs, want = edge_streams
    assert mb.batch_tags(streams, rs, plan_of(shapes, groups)) == want


def test_model_rejects_a_wrong_exponent(edge_streams):
    """The comparison is live: every segment folded in one power of R too low changes every tag."""
    shapes, streams, rs, want = edge_streams
    wrong = mb.batch_tags(streams, rs, plan_of(shapes, 3), exp_shift=1)
    assert all(w != t for w, t in zip(wrong, want))


@pytest.mark.parametrize("groups", mb.GROUPS)
def test_plan_properties_of_the_edge_batch(groups):
    from suruga_amd import msg

    shapes = mb.edge_shapes()
    mb.check_plan(plan_of(shapes, groups), shapes, groups, msg.plan_for)


def test_edge_batch_shows_every_situation():
    """Asserted from the plan: over the group settings of the GPU test the edge
    batch holds every situation it was built for (tests/test_gpu_msg_batch.py
    asserts the same before it runs)."""
    shapes = mb.edge_shapes()
    per_setting = {g: mb.plan_features(plan_of(shapes, g)) for g in mb.GROUPS}
    assert set().union(*per_setting.values()) == mb.FEATURES, per_setting
    assert "group from inside one message to inside another, a whole one between" in per_setting[5]
    assert "message whose every tile is its own segment" in per_setting[0]


def test_plan_of_no_message_and_of_one_empty_message():
    from suruga_amd import msg

    mb.check_plan(plan_of([], 0), [], 0, msg.plan_for)
    p = plan_of([(0, 0)], 0)
    mb.check_plan(p, [(0, 0)], 0, msg.plan_for)
    assert (p["tiles"], p["groups"], p["segments"]) == (1, 1, 1)
    assert p["segs"] == [{"msg": 0, "tile_begin": 0, "tile_end": 1, "group": 0}]


@pytest.mark.parametrize("groups", [0, 7, 1])
def test_plan_of_many_small_messages(groups):
    from suruga_amd import msg

    shapes = mb.many_shapes()
    p = plan_of(shapes, groups)
    mb.check_plan(p, shapes, groups, msg.plan_for)
    assert p["tiles"] == 3000 and p["groups"] == (groups or 1000) and p["segments"] == 3000


def test_plan_of_a_long_message_has_more_than_256_segments():
    from suruga_amd import msg

    shapes = mb.long_shapes()
    p = plan_of(shapes, 0)
    mb.check_plan(p, shapes, 0, msg.plan_for)
    assert max(cnt for _, cnt in p["msg_segs"]) > 256


def test_plan_rejects_a_length_above_the_bound():
    import ctypes as C

    from suruga_amd import _native as N
    from suruga_amd import msg

    with pytest.raises(N.NativeError) as e:
        msg.batch_plan_for([10, N.SG_MSG_MAX_LEN + 1], [0, 0])
    assert e.value.code == N.SG_E_ARG
    with pytest.raises(N.NativeError):
        msg.batch_plan_for([10, 10], [0, N.SG_MSG_MAX_LEN + 1])
    msg.batch_plan_for([N.SG_MSG_MAX_LEN], [N.SG_MSG_MAX_LEN])  # the bound itself is planned
    lib = N.load()
    n = (C.c_uint64 * 2)(1, 2)
    plan = N.SgMsgBatchPlan()
    assert lib.sg_msg_batch_plan_for(n, n, 2, 0, None, None, None, 0, None, None) == N.SG_E_ARG  # no plan
    assert lib.sg_msg_batch_plan_for(None, n, 2, 0, C.byref(plan), None, None, 0, None, None) == N.SG_E_ARG
    segs = (N.SgMsgSeg * 1)()
    assert lib.sg_msg_batch_plan_for(n, n, 2, 0, C.byref(plan), None, segs, 1, None, None) == N.SG_E_ARG  # no room
    assert lib.sg_msg_batch_plan_for(n, n, 2, 0, C.byref(plan), None, None, 0, None, None) == N.SG_OK
    assert (plan.tiles, plan.groups, plan.segments) == (2, 2, 2)
