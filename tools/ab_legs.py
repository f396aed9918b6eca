"""What the alternating-leg bench tools share (rfc_batch_bench.py, tls13_batch_bench.py,
msg_bench.py, msg_batch_bench.py): the start of a run, the timed loop over the legs,
the clock sampled beside it, a leg's summary and the choice of records to check.

The method: the legs of a comparison run launch by launch in one process, every leg
once per round, so they share the clock the board holds; every round runs them in
another order (a seeded shuffle), so that no leg always follows the same one -- the
board is power-managed, and a launch behind a slow leg finds a higher clock than one
behind a fast leg.  Each launch is timed by HIP events around the call.
"""
from __future__ import annotations

import contextlib
import random
import statistics
import time


def prelude(tool: str, reps: int, warmup: int):
    """Build the library if it is stale and insist on the GPU: (the head of the tool's
    JSON line, the PCI bus id of device 0 for clock())."""
    import torch

    from suruga_amd import _build, _native

    _build.build_library()
    assert torch.cuda.is_available(), f"{tool} needs an MI355X"
    props = torch.cuda.get_device_properties(0)
    bus = f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}.0"
    return {"tool": tool, "device": torch.cuda.get_device_name(0), "lib": _native.loaded_info(), "reps": reps,
            "warmup": warmup}, bus


def summary(ms: list, nbytes: int) -> dict:
    """Median, extremes and spread = (max - min) / median of a leg's launches; GiB/s of nbytes at the median."""
    med = statistics.median(ms)
    return {"ms": round(med, 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5),
            "spread": round((max(ms) - min(ms)) / med, 4), "gib_s": round(nbytes / 2**30 / (med * 1e-3), 1),
            "launches": len(ms)}


def timed_legs(legs: dict, reps: int, warmup: int, stream=None) -> dict:
    """name -> the milliseconds of `reps` launches after `warmup` rounds.  legs: name -> fn,
    or (pre, fn) where pre() runs ahead of the timed region; every leg once per round in
    the round's shuffled order; the events are recorded on `stream` (None: the current one)."""
    import torch

    order = [(name, leg if isinstance(leg, tuple) else (None, leg)) for name, leg in legs.items()]
    times = {name: [] for name, _ in order}
    for rep in range(warmup + reps):
        for name, (pre, fn) in random.Random(rep).sample(order, len(order)):
            if pre:
                pre()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return times


@contextlib.contextmanager
def clock(bus: str, on: bool = True):
    """Samples the shader clock and board power (sysfs, read only) while the block runs;
    the dict it yields holds sclk_mhz, board_power_w and power_cap_w once the block is left
    (on=False: nothing is sampled and it stays empty)."""
    from suruga_amd import devmon

    out: dict = {}
    sampler = devmon.Sampler(bus, period=0.002).start() if on else None
    t0 = time.perf_counter()
    try:
        yield out
    finally:
        if sampler:
            clk = sampler.stop(t0, time.perf_counter())
            out.update(sclk_mhz=clk["sclk_mhz"], board_power_w=clk["board_power_w"], power_cap_w=clk.get("power_cap_w"))


def sample_indices(count: int, sample: int) -> list:
    """The records a tool compares with its reference: the first two, the middle one, the
    last one and `sample` more spread by a multiplicative hash."""
    return sorted({0, 1 % count, count // 2, count - 1} | {(i * 2654435761) % count for i in range(sample)})
