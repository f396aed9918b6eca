"""GPU parity of the message batch (sg_seal_msg_batch / sg_open_msg_batch): many
messages of any length on one grid, every byte against oracle.seal /
oracle.open per message.  Every call runs on sentinel buffers
(msg_batch_support.run) and the whole output buffer, the whole input buffer and
the status array with 64 bytes behind it are compared, so a stray store shows
in every test, not only in the footprint one."""
from __future__ import annotations

import pytest

import mac_forge as mf
import msg_batch_support as mb
from gpu_support import groups  # noqa: F401  (a fixture)
from suruga_amd._native import SG_E_ARG

pytestmark = pytest.mark.gpu


def plan_of(shapes, g):
    from suruga_amd import msg

    return msg.batch_plan_for([n for _, n in shapes], [a for a, _ in shapes], g)


def round_trip(oracle, msgs, where, **kw):
    """Seal and open of msgs; both whole-buffer exact."""
    mb.run(mb.KEYS, *mb.seal_case(msgs), open_=False, **kw).check(where=(*where, "seal"))
    args, st = mb.open_case(oracle, msgs)
    mb.run(mb.KEYS, *args, open_=True, **kw).check(st, where=(*where, "open"))


def test_edge_batch_covers_its_situations(gpu):
    """(The gpu fixture first, as everywhere: it imports torch ahead of the library,
    so that both use the one HIP runtime torch brings.)
    From the plan, not from arithmetic here: over the group settings below the
    edge batch has a group with two whole messages, a message in several
    segments, a cut on a message boundary, a group from inside one message to
    inside another with a whole one between (groups = 5) and a message whose
    every tile is its own segment (groups = 0)."""
    shapes = mb.edge_shapes()
    seen = {g: mb.plan_features(plan_of(shapes, g)) for g in mb.GROUPS}
    assert set().union(*seen.values()) == mb.FEATURES, seen
    assert "group from inside one message to inside another, a whole one between" in seen[5]
    assert "message whose every tile is its own segment" in seen[0]


@pytest.mark.parametrize("g", mb.GROUPS)
def test_edge_batch(gpu, oracle, groups, g):
    """Thirteen messages, 30 tiles, a distinct key index out of 4 and a distinct
    nonce each, in / out / ad offsets cycling through 0, 1, 3."""
    groups(g)
    msgs = mb.messages(oracle, mb.edge_shapes())
    assert len({m.nonce for m in msgs}) == len(msgs) and {m.kidx for m in msgs} == set(range(mb.NUM_KEYS))
    round_trip(oracle, msgs, (g,))


def test_more_than_256_segments_in_one_message(gpu, oracle, groups):
    groups(0)
    shapes = mb.long_shapes()
    assert max(cnt for _, cnt in plan_of(shapes, 0)["msg_segs"]) > 256
    round_trip(oracle, mb.messages(oracle, shapes, 1), ("long",))


def test_more_messages_than_groups(gpu, oracle, groups):
    groups(0)
    shapes = mb.many_shapes()
    p = plan_of(shapes, 0)
    assert len(shapes) == 3000 > p["groups"] and p["tiles_per_group"] == 3
    round_trip(oracle, mb.messages(oracle, shapes, 2), ("many",))


TAMPER = {2: "tag", 4: "first", 5: "last", 8: "ad", 11: "last", 12: "first"}
SHORT = (6,)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("g", [3, 0])
def test_open_tampered_and_short(gpu, oracle, groups, g, keep):
    """Per-message status; failed outputs zero, or with SG_MSG_KEEP_FAILED the
    oracle's unauthenticated decryption; the short message's output untouched;
    every other message intact."""
    groups(g)
    msgs = mb.messages(oracle, mb.edge_shapes())
    args, st = mb.open_case(oracle, msgs, TAMPER, SHORT, keep)
    assert sorted(i for i, s in enumerate(st) if s == 1) == sorted(TAMPER) and st[6] == 2 and st.count(0) == 6
    mb.run(mb.KEYS, *args, open_=True, keep=keep).check(st, where=(g, keep))


@pytest.mark.parametrize("g", [2, 0])
def test_in_place(gpu, oracle, groups, g):
    """out == in for every second message, both directions, with a tampered one among them."""
    groups(g)
    msgs = mb.messages(oracle, mb.edge_shapes())
    every_second = set(range(0, len(msgs), 2))
    round_trip(oracle, msgs, (g, "in place"), in_place=every_second)
    args, st = mb.open_case(oracle, msgs, {4: "first", 5: "tag"})
    mb.run(mb.KEYS, *args, open_=True, in_place=every_second).check(st, where=(g, "in place tampered"))


@pytest.mark.parametrize("what", ["seal", "open", "open tampered", "open tampered keep_failed"])
def test_footprint(gpu, oracle, groups, what):
    """The messages back to back in sentinel buffers, gaps cycling through
    footprint.GAPS, every result's edge bytes off the sentinel: not one byte
    outside a message's own range changes, in any of the three buffers."""
    groups(0)
    msgs = mb.messages(oracle, mb.edge_shapes())
    if what == "seal":
        mb.run(mb.KEYS, *mb.seal_case(msgs), open_=False, layout=mb.gap_layout, strict=True).check(where=(what,))
        return
    keep = what.endswith("keep_failed")
    args, st = mb.open_case(oracle, msgs, TAMPER if "tampered" in what else None, SHORT, keep)
    mb.run(mb.KEYS, *args, open_=True, keep=keep, layout=mb.gap_layout, strict=True).check(st, where=(what,))


def forged_round(oracle, msgs, where):
    keys = mf.KEY * mb.NUM_KEYS
    mb.run(keys, *mb.seal_case(msgs), open_=False).check(where=(*where, "seal"))
    args, st = mb.open_case(oracle, msgs)
    mb.run(keys, *args, open_=True).check(st, where=(*where, "open"))
    args, st = mb.open_case(oracle, msgs, {i: "tag" for i in range(len(msgs))})
    mb.run(keys, *args, open_=True).check(st, where=(*where, "open tag + 1"))


def test_mac_edge_states_whole_message(gpu, oracle, groups):
    """mac_forge.msg_a(): messages whose whole-stream accumulator is forged to the
    edge values (0, p - 1, 2^128, ...), all lengths in one batch, through the
    batch's finish (wave sum, carry, tag words, + s)."""
    groups(0)
    cases = [c for v in mf.msg_a().values() for c in v]
    forged_round(oracle, mb.forged_messages(cases), ("msg_a",))


@pytest.mark.parametrize("g", mf.MSG_GROUPS_B)
def test_mac_edge_states_lane_terms(gpu, oracle, groups, g):
    """mac_forge.msg_b(): every lane term of the single-message kernel forged to
    -1 or 0.  The lane terms carry over to the batch, because a message's tile
    geometry is the single call's and a lane keeps blocks 4 l .. 4 l + 3 of every
    tile.  The "mg" cases forge the single call's GROUP partials; the batch cuts
    the four messages' 16 tiles into its own segments, which are not expected to
    coincide with those groups: they run here as ordinary messages."""
    groups(g)
    forged_round(oracle, mb.forged_messages(mf.msg_b()[g]), ("msg_b", g))


def test_two_streams_with_caller_workspaces(gpu, oracle, groups):
    """Two batches enqueued on two streams, each with its own workspace, then synchronised."""
    import torch

    from suruga_amd import msg

    groups(0)
    a, b = mb.messages(oracle, mb.edge_shapes()), mb.messages(oracle, mb.long_shapes()[2:] + mb.edge_shapes()[:5], 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ws = [torch.empty(msg.batch_workspace_size(len(m)), dtype=torch.uint8, device="cuda") for m in (a, b)]
    torch.cuda.synchronize()
    wait_a = mb.run(mb.KEYS, *mb.seal_case(a), open_=False, stream=s1, workspace=ws[0], sync=False)
    wait_b = mb.run(mb.KEYS, *mb.seal_case(b), open_=False, stream=s2, workspace=ws[1], sync=False)
    wait_a().check(where=("stream 1",))
    wait_b().check(where=("stream 2",))


def test_stream_capture_is_refused(gpu, oracle):
    """The table upload is a copy a capture cannot record: SG_E_ARG, with a caller workspace too."""
    import torch

    from suruga_amd import _native as N
    from suruga_amd import msg

    msgs = mb.messages(oracle, mb.edge_shapes()[:2])
    keys = torch.zeros(mb.NUM_KEYS, 32, dtype=torch.uint8, device="cuda")
    inp = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ws = torch.empty(msg.batch_workspace_size(1), dtype=torch.uint8, device="cuda")
    items = [msg.MsgItem(0, msgs[0].nonce, inp, out, in_len=8)]
    msg.seal_msgs(keys, items, workspace=ws)  # warm: the code objects are loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g):
        out.zero_()  # (the capture records something, whatever the call below does)
        try:
            msg.seal_msgs(keys, items, stream=torch.cuda.current_stream(), workspace=ws)
        except N.NativeError as e:
            err = e
    torch.cuda.synchronize()
    assert err is not None and err.code == SG_E_ARG and "capture" in str(err)
