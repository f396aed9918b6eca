"""What the message-batch tests share (tests/test_msg_batch_model.py and
tests/test_msg_batch_abi.py on the CPU, tests/test_gpu_msg_batch.py on the GPU)
-- TEST INFRASTRUCTURE ONLY.

* the edge batch of thirteen messages and the other shapes,
* the batch decomposition restated in Python integers from the exported plan,
* what the plan must show over the runs of the edge batch,
* messages sealed by the oracle (cached), and a runner that lays a batch out in
  sentinel buffers (footprint.sentinel), calls sg_seal_msg_batch /
  sg_open_msg_batch once and hands back whole buffers with the images they
  must equal.

Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

import footprint as fp

P1305 = (1 << 130) - 5
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
TB = 16320  # tile bytes; test_msg_batch_model.py holds it against the plan
GROUPS = (1, 2, 3, 5, 7, 0)
NUM_KEYS = 4
KEYS = b"".join(hashlib.sha256(b"message batch key %d" % i).digest() for i in range(NUM_KEYS))
OFFS = (0, 1, 3)


def edge_shapes():
    """Thirteen messages, 30 tiles, as (adlen, n); L = adlen + 16 + n."""
    return [(0, 0), (13, 1),
            (13, TB - 30), (13, TB - 29), (13, TB - 28),          # L = TB - 1, TB, TB + 1
            (8, 2 * TB - 24 - 17), (8, 2 * TB - 24), (8, 2 * TB - 24 + 17),
            (7, 3 * TB - 18),                                      # L = 3 TB + 5
            (0, TB - 13),                                          # L = TB + 3: le64(n) across two MAC blocks
            (TB + 5, 0), (2 * TB + 9, 100), (256, 5 * TB)]


def long_shapes():
    """One message of 300 tiles (more than 256 segments on the automatic grid) and five small ones."""
    return [(13, 40), (13, 300 * TB - 29), (0, 0), (5, TB), (13, 1000), (0, 17)]


def many_shapes():
    """3,000 messages of 0..200 bytes, AD of 0..20."""
    rng = np.random.default_rng(3000)
    return [(int(a), int(n)) for a, n in zip(rng.integers(0, 21, 3000), rng.integers(0, 201, 3000))]


def tiles_of(adlen: int, n: int) -> int:
    return max(1, -(-(adlen + 16 + n) // TB))


def rnd(tag: str, n: int) -> bytes:
    """n bytes from SHA-256 of the tag: the streams and Poly1305 keys of the CPU models."""
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(f"{tag}:{i}".encode()).digest()
        i += 1
    return out[:n]


# ---------------------------------------------------------------------------
# the C batch on the host (the argument checks never dereference a device pointer)
# ---------------------------------------------------------------------------
def batch(count=2, n=100, adlen=13):
    """A well-formed seal batch on made-up device addresses, its items and a fitting workspace size."""
    from suruga_amd import _native as N

    items = (N.SgMsgItem * max(count, 1))()
    for i in range(count):
        it = items[i]
        it.key_index = i % 2
        it.ad, it.ad_len = 0x100000 + 0x1000 * i, adlen
        it.in_, it.in_len = 0x200000 + 0x10000 * i, n
        it.out = 0x400000 + 0x10000 * i
    b = N.SgMsgBatch()
    b.count, b.flags, b.keys, b.num_keys, b.items = count, 0, 0x1000, 2, items
    b.status = 0x2000
    b.stream = None
    b.workspace, b.workspace_size = 0x800000, N.load().sg_msg_batch_workspace_size(count)
    return b, items


def rejected(lib, b, open_=False, text=None):
    """The call answers SG_E_ARG, with `text` in sg_last_error where one is given."""
    import ctypes as C

    from suruga_amd._native import SG_E_ARG

    rc = (lib.sg_open_msg_batch if open_ else lib.sg_seal_msg_batch)(C.byref(b))
    assert rc == SG_E_ARG, rc
    if text:
        assert text.encode() in lib.sg_last_error(), lib.sg_last_error()


# ---------------------------------------------------------------------------
# the decomposition in Python integers
# ---------------------------------------------------------------------------
def batch_tags(streams, rs, plan: dict, exp_shift: int = 0):
    """The tag of every message as the batch kernels compute it: per-segment
    chains from h = 0 over the segment's tiles (each tile's Horner chain from
    zero, folded with R = r^K), the per-message sum of H_seg R^(T_m - b), + s
    (exp_shift: a wrong exponent, for the test that the comparison is live)."""
    segs = plan["segs"]
    out = []
    for m, (stream, (r16, s16)) in enumerate(zip(streams, rs)):
        r = int.from_bytes(r16, "little") & CLAMP
        pm = plan["msgs"][m]
        K, T, z, B = pm["tile_blocks"], pm["tiles"], pm["zero_blocks"], pm["mac_blocks"]
        assert B == (len(stream) + 15) // 16 and z + B == T * K

        def block(v: int) -> int:
            if v < z:
                return 0  # virtual: value 0, no pad bit
            chunk = stream[16 * (v - z):16 * (v - z) + 16]
            return int.from_bytes(chunk, "little") | (1 << (8 * len(chunk)))

        R = pow(r, K, P1305)
        first, cnt = plan["msg_segs"][m]
        total = 0
        for sg in segs[first:first + cnt]:
            assert sg["msg"] == m
            H = 0
            for t in range(sg["tile_begin"], sg["tile_end"]):
                h = 0
                for i in range(K):
                    h = (h + block(t * K + i)) * r % P1305
                H = (H * R + h) % P1305
            total = (total + H * pow(R, T - sg["tile_end"] - exp_shift, P1305)) % P1305
        out.append(((total + int.from_bytes(s16, "little")) % (1 << 128)).to_bytes(16, "little"))
    return out


def check_plan(plan: dict, shapes, groups: int, single_plan):
    """The plan's properties; single_plan(n, adlen, groups) is msg.plan_for."""
    count = len(shapes)
    assert len(plan["msgs"]) == len(plan["msg_segs"]) == count
    for (adlen, n), pm in zip(shapes, plan["msgs"]):
        assert pm == single_plan(n, adlen, groups), (adlen, n)
    TT = sum(pm["tiles"] for pm in plan["msgs"])
    assert plan["tiles"] == TT
    G, per = plan["groups"], plan["tiles_per_group"]
    if count == 0:
        assert (TT, G, plan["segments"]) == (0, 0, 0)
        return
    want_g = min(TT, groups if groups else 1024)
    assert per == -(-TT // want_g) and G == -(-TT // per) and 1 <= G <= want_g
    segs = plan["segs"]
    assert len(segs) == plan["segments"] <= G + count - 1
    # the segments partition the global tiles exactly once, in order, none across a message
    base = np.concatenate([[0], np.cumsum([pm["tiles"] for pm in plan["msgs"]])])
    pos = 0
    for sg in segs:
        m = sg["msg"]
        assert 0 <= sg["tile_begin"] < sg["tile_end"] <= plan["msgs"][m]["tiles"], sg
        assert int(base[m]) + sg["tile_begin"] == pos, sg
        pos = int(base[m]) + sg["tile_end"]
        # the whole segment lies in its group's run
        assert sg["group"] * per <= int(base[m]) + sg["tile_begin"] and pos <= min(TT, (sg["group"] + 1) * per), sg
    assert pos == TT
    # group runs: contiguous, none empty, covering [g per, min(TT, (g + 1) per))
    nxt = 0
    for g, (first, cnt) in enumerate(plan["group_segs"]):
        assert cnt >= 1 and first == nxt, (g, first, cnt)
        run = segs[first:first + cnt]
        assert all(sg["group"] == g for sg in run)
        assert int(base[run[0]["msg"]]) + run[0]["tile_begin"] == g * per
        assert int(base[run[-1]["msg"]]) + run[-1]["tile_end"] == min(TT, (g + 1) * per)
        nxt = first + cnt
    assert nxt == len(segs)
    nxt = 0
    for m, (first, cnt) in enumerate(plan["msg_segs"]):
        assert cnt >= 1 and first == nxt and all(sg["msg"] == m for sg in segs[first:first + cnt]), m
        nxt = first + cnt
    assert nxt == len(segs)


def plan_features(plan: dict) -> set:
    """Which of the situations the edge batch is there for this plan holds."""
    segs, msgs = plan["segs"], plan["msgs"]
    whole = lambda sg: sg["tile_begin"] == 0 and sg["tile_end"] == msgs[sg["msg"]]["tiles"]
    out = set()
    for first, cnt in plan["group_segs"]:
        run = segs[first:first + cnt]
        if sum(whole(sg) for sg in run) >= 2:
            out.add("group with two whole messages")
        if (len(run) >= 3 and run[0]["tile_begin"] > 0 and run[-1]["tile_end"] < msgs[run[-1]["msg"]]["tiles"]
                and any(whole(sg) for sg in run[1:-1])):
            out.add("group from inside one message to inside another, a whole one between")
    for m, (first, cnt) in enumerate(plan["msg_segs"]):
        if cnt >= 2:
            out.add("message cut into segments")
        if msgs[m]["tiles"] >= 2 and cnt == msgs[m]["tiles"]:
            out.add("message whose every tile is its own segment")
    for a, b in zip(segs, segs[1:]):
        if a["group"] != b["group"] and a["msg"] != b["msg"]:
            out.add("cut on a message boundary")
    return out


FEATURES = {"group with two whole messages", "message cut into segments", "cut on a message boundary",
            "group from inside one message to inside another, a whole one between",
            "message whose every tile is its own segment"}


# ---------------------------------------------------------------------------
# messages
# ---------------------------------------------------------------------------
@dataclass
class Msg:
    kidx: int
    nonce: bytes
    ad: bytes
    pt: bytes
    sealed: bytes
    table: bytes = KEYS  # the call's key table

    @property
    def key(self) -> bytes:
        return self.table[32 * self.kidx:32 * self.kidx + 32]


_cache: dict = {}


def messages(oracle, shapes, tag: int = 0):
    """Messages of the shapes, each under key i % 4 and its own nonce, sealed by the oracle once."""
    key = (tuple(shapes), tag)
    if key not in _cache:
        rng = np.random.default_rng([len(shapes), tag, 77])
        out = []
        for i, (adlen, n) in enumerate(shapes):
            nonce = i.to_bytes(4, "little") + rng.bytes(4)
            m = Msg(i % NUM_KEYS, nonce, rng.bytes(adlen), rng.bytes(n), b"")
            m.sealed = oracle.seal(m.key, nonce, m.pt, m.ad)
            out.append(m)
        _cache[key] = out
    return _cache[key]


def forged_messages(cases):
    """mac_forge records (all under mac_forge.KEY) as messages of key table [KEY] * 4."""
    import mac_forge as mf

    return [Msg(i % NUM_KEYS, f.nonce, f.ad, f.pt, f.want, mf.KEY * NUM_KEYS)
            for i, f in enumerate(mf.make(*c) for c in cases)]


# ---------------------------------------------------------------------------
# one call on sentinel buffers
# ---------------------------------------------------------------------------
def cycle_layout(lens, phase: int):
    """Every range 16-byte aligned plus OFFS[(i + phase) % 3], 16 spare bytes behind it."""
    off, pos = [], fp.MARGIN
    for i, n in enumerate(lens):
        pos = fp.round_up(pos, 16) + OFFS[(i + phase) % 3]
        off.append(pos)
        pos += int(n) + 16
    return off, fp.round_up(pos, 16) + fp.MARGIN


def gap_layout(lens):
    """footprint.layout's ranges: margins, gaps cycling through footprint.GAPS."""
    off, _, size, _ = fp.layout(lens, lens)
    return [int(o) for o in off], size


def run(keys_h: bytes, kidx, nonces, ads, inputs, out_lens, results, *, open_: bool, layout=cycle_layout,
        in_place=(), keep=False, stream=None, workspace=None, salt: int = 0x11, strict: bool = False,
        sync: bool = True):
    """One sg_seal_msg_batch / sg_open_msg_batch call.  Message i reads inputs[i]
    and ads[i], has a nominal output range of out_lens[i] bytes and must leave
    results[i] there (None: untouched).  Messages in `in_place` get out == in.
    strict: the salt is searched so that every result's first and last byte
    differ from the sentinel under them (footprint.pick_salt).
    Returns a footprint.Outcome whose check takes the statuses (none: a seal, which
    writes no status); with sync False, a function that waits and returns it."""
    from gpu_support import dev_bytes, dev_u8
    from suruga_amd import msg

    count = len(inputs)
    in_slot = [max(len(inputs[i]), out_lens[i]) if i in in_place else len(inputs[i]) for i in range(count)]
    if layout is cycle_layout:
        in_off, in_size = cycle_layout(in_slot, 0)
        out_off, out_size = cycle_layout(out_lens, 1)
        ad_off, ad_size = cycle_layout([len(a) for a in ads], 2)
    else:
        in_off, in_size = layout(in_slot)
        out_off, out_size = layout(out_lens)
        ad_off, ad_size = layout([len(a) for a in ads])
    parts = [(out_off[i], results[i]) for i in range(count) if i not in in_place and results[i] is not None]
    if strict:
        salt, _ = fp.pick_salt(out_size, parts, salt)
    in_img = fp.image(in_size, salt + 1, zip(in_off, inputs))
    want_inp = in_img.copy()
    for i in in_place:
        if results[i] is not None:
            want_inp[in_off[i]:in_off[i] + len(results[i])] = np.frombuffer(bytes(results[i]), dtype=np.uint8)

    def call(d):
        ad_t, keys_t = dev_u8(fp.image(ad_size, salt + 2, zip(ad_off, ads))), dev_bytes(keys_h).view(-1, 32)
        items = [msg.MsgItem(kidx[i], nonces[i], d["inp"][in_off[i]:],
                             d["inp"][in_off[i]:] if i in in_place else d["out"][out_off[i]:],
                             ad=ad_t[ad_off[i]:], in_len=len(inputs[i]), ad_len=len(ads[i])) for i in range(count)]
        if open_:
            msg.open_msgs(keys_t, items, d["status"], keep_failed=keep, stream=stream, workspace=workspace)
        else:
            msg.seal_msgs(keys_t, items, stream=stream, workspace=workspace)
        return ad_t, keys_t  # (Outcome.ret: they live until the work is done)

    return fp.run_whole(call, in_img, fp.sentinel(out_size, salt), fp.image(out_size, salt, parts),
                        [(out_off[i], out_off[i] + out_lens[i]) for i in range(count)], want_inp=want_inp,
                        in_ranges=[(in_off[i], in_off[i] + in_slot[i]) for i in range(count)],
                        arrays={"status": np.full(count + fp.ARRAY_PAD, 0xFF, dtype=np.uint8)}, sync=sync)


def seal_case(msgs):
    """(kidx, nonces, ads, inputs, out_lens, results) of a seal of msgs."""
    return ([m.kidx for m in msgs], [m.nonce for m in msgs], [m.ad for m in msgs], [m.pt for m in msgs],
            [len(m.pt) + 16 for m in msgs], [m.sealed for m in msgs])


def open_case(oracle, msgs, tamper=None, short=(), keep=False):
    """The open of msgs' sealed bytes: tamper = {i: "tag" | "first" | "last" | "ad"},
    short = indices whose input is cut to 15 bytes (nominal output 24 bytes,
    untouched).  Returns (args of run, statuses)."""
    tamper = tamper or {}
    ads, inputs, out_lens, results, st = [], [], [], [], []
    for i, m in enumerate(msgs):
        ad, ct, n = m.ad, bytearray(m.sealed), len(m.pt)
        if i in short:
            ads.append(ad)
            inputs.append((bytes(ct) + bytes(15))[:15])
            out_lens.append(24)
            results.append(None)
            st.append(2)
            continue
        how = tamper.get(i)
        if how == "ad":
            ad = bytes([ad[0] ^ 0x10]) + ad[1:]
        elif how is not None:
            ct[{"tag": n + 9, "first": 0, "last": n - 1}[how]] ^= 0x01
        ads.append(ad)
        inputs.append(bytes(ct))
        out_lens.append(n)
        if how is None:
            results.append(m.pt)
            st.append(0)
        else:
            rc, plain = oracle.open(m.key, m.nonce, bytes(ct), ad)
            assert rc == 1
            results.append(plain if keep else bytes(n))
            st.append(1)
    return ([m.kidx for m in msgs], [m.nonce for m in msgs], ads, inputs, out_lens, results), st
