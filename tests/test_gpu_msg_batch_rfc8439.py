"""GPU parity of the message batch in RFC 8439 (SG_MSG_RFC8439 on
sg_seal_msg_batch / sg_open_msg_batch): one call of forty messages -- the edge
shapes of the padded stream, two messages of 3 T + 5 bytes, a run of twenty
empty ones; three keys, forty different 12-byte nonces -- against the reference
(tests/rfc8439_ref.py, tied to OpenSSL by tests/test_rfc8439_ref.py) and against
a loop of single calls.

The calls run through msg_batch_support.run: sentinel buffers, the whole
output, input and status buffers compared afterwards."""
from __future__ import annotations

import contextlib
import functools

import pytest

import msg_batch_support as mbs
import rfc8439_ref as ref
from gpu_support import dev_bytes, groups, host_bytes  # noqa: F401  (groups: a fixture)

pytestmark = pytest.mark.gpu

GROUPS = (1, 3, 0)
LAYOUTS = {"cycle": mbs.cycle_layout, "gap": mbs.gap_layout}


@contextlib.contextmanager
def rfc8439_calls():
    """msg_batch_support.run calls msg.seal_msgs / msg.open_msgs: inside this block they speak RFC 8439."""
    from suruga_amd import msg

    seal, open_ = msg.seal_msgs, msg.open_msgs
    msg.seal_msgs = functools.partial(seal, rfc8439=True)
    msg.open_msgs = functools.partial(open_, rfc8439=True)
    try:
        yield
    finally:
        msg.seal_msgs, msg.open_msgs = seal, open_


def run(*args, **kw):
    with rfc8439_calls():
        return mbs.run(ref.KEYS, *args, **kw)


class Checker:
    """What msg_batch_support.open_case asks of a checker."""

    open = staticmethod(ref.open)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("g", GROUPS)
def test_seal(gpu, groups, g, layout):
    groups(g)
    msgs = ref.batch_messages()
    in_place = {5, 9, 12, 21} if layout == "cycle" else ()
    run(*mbs.seal_case(msgs), open_=False, layout=LAYOUTS[layout], in_place=in_place, strict=True).check(
        where=(g, layout))


@pytest.mark.parametrize("g", GROUPS)
def test_batch_is_the_loop_of_single_calls(gpu, groups, g):
    """Message by message through sg_seal_msg_dev / sg_open_msg_dev with the flag: the
    bytes the batch gave (test_seal), which are the reference's."""
    import torch

    from suruga_amd import msg

    groups(g)
    keys_t = dev_bytes(ref.KEYS).view(-1, 32)
    st = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, m in enumerate(ref.batch_messages()):
        n = len(m.pt)
        buf = dev_bytes(m.pt + bytes(16))
        ad = dev_bytes(m.ad)[:len(m.ad)]
        msg.seal_msg(keys_t[m.kidx], m.nonce, buf, buf, ad=ad, in_len=n, stream=0, rfc8439=True)
        assert host_bytes(buf) == m.sealed, (g, i)
        assert msg.open_(keys_t[m.kidx], m.nonce, buf, buf, st, ad=ad, in_len=n + 16, stream=0, rfc8439=True) == 0
        assert int(st.item()) == 0 and host_bytes(buf)[:n] == m.pt, (g, i)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("g", GROUPS)
def test_open_with_tampered_and_short_messages(gpu, groups, g, keep):
    """Two tampered messages (the ciphertext of a 3 T + 5 byte one, the AD of an
    edge shape), one tampered tag and one input of 15 bytes among the forty."""
    groups(g)
    msgs = ref.batch_messages()
    tamper = {9: "last", 11: "ad", 4: "tag"}
    assert len(msgs[9].pt) == 3 * ref.TB + 5 and len(msgs[11].ad) > 0
    case, st = mbs.open_case(Checker, msgs, tamper=tamper, short=(17,), keep=keep)
    assert [s for s in st if s] == [1, 1, 1, 2] and st[17] == 2
    run(*case, open_=True, layout=mbs.gap_layout if keep else mbs.cycle_layout, in_place={9, 30} if not keep else (),
        keep=keep).check(st, where=(g, keep))


def test_open_of_everything_sealed(gpu, groups):
    groups(0)
    msgs = ref.batch_messages()
    case, st = mbs.open_case(Checker, msgs)
    assert not any(st)
    run(*case, open_=True, strict=True).check(st)


def test_draft_call_on_the_same_items_is_still_the_draft(gpu, oracle):
    """Without the flag the same structs, garbage in every nonce_hi, give the
    draft's bytes: the 8 bytes of `nonce` alone count."""
    import ctypes as C

    import torch

    from suruga_amd import msg

    msgs = ref.batch_messages()[:12]
    keys_t = dev_bytes(ref.KEYS).view(-1, 32)
    bufs = [dev_bytes(m.pt + bytes(16)) for m in msgs]
    ads = [dev_bytes(m.ad)[:len(m.ad)] for m in msgs]
    items = [msg.MsgItem(m.kidx, m.nonce[4:], b, b, ad=a, in_len=len(m.pt)) for m, b, a in zip(msgs, bufs, ads)]
    b = msg._msg_batch(keys_t, items, None, False, 0, None)
    for i, m in enumerate(msgs):
        b.items[i].nonce_hi[:] = m.nonce[:4] if i % 2 else b"\xff" * 4
    assert b.flags == 0 and gpu.sg_seal_msg_batch(C.byref(b)) == 0
    torch.cuda.synchronize()
    for i, (m, buf) in enumerate(zip(msgs, bufs)):
        assert host_bytes(buf) == oracle.seal(m.key, m.nonce[4:], m.pt, m.ad), i
