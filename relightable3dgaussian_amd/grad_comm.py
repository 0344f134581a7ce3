"""The gradient-bucket all-reduces of the data-parallel stage-2 iteration (fused_step.FusedStage2Step holds one BucketComm):
issuing a collective -- RCCL's, or its priced rehearsal on one rank -- waiting for it, and the measurement of both for
bench.py (what the compute stream stalls on, and a per-bucket table)."""
import os

import torch

from . import _lib
from .fused_base import shared_stream


def _fake_comm_gbs():
    v = os.environ.get("R3DG_DP_FAKE_COMM_GBS")
    return float(v) if v else None


class _FakeCommHandle:
    """What torch.distributed's Work is to the callers of BucketComm.allreduce_async: wait() orders the current stream behind
    the (priced) end of the collective."""

    def __init__(self, event, begin=None):
        self.event, self.begin = event, begin

    def wait(self):
        torch.cuda.current_stream().wait_event(self.event)

    def _get_duration(self):
        """ms the priced collective held the communication stream (same name as torch.distributed.Work's)."""
        if self.begin is None:
            raise RuntimeError("the priced collective was not timed")
        return self.begin.elapsed_time(self.event)


class BucketComm:
    """`it` (every call): the iteration the bucket belongs to, for the measurement's bookkeeping."""
    def __init__(self, dev, group, world, dp):
        self.dev, self.group, self.world, self.dp = dev, group, world, dp
        self.measure_comm = False                   # bench.py: time the main stream spends waiting for all-reduce buckets
        # with measure_comm: every n-th iteration's buckets get the two probe events (0 = never; R3DG_COMM_PROBE_EVERY)
        self.comm_probe_every = int(os.environ.get("R3DG_COMM_PROBE_EVERY", "4"))
        self._comm_events = []                      # (iteration, wait begin, wait end, bucket, on a side stream): exposed_comm_ms()
        self._bucket_events = []                    # (iteration, bucket, bytes, ready event, work handle): comm_table()
        self._released = {}                         # (iteration, bucket) -> the event behind its wait (exposed_comm_ms -> comm_table)

    def allreduce_async(self, flat, name, it):
        """Sum `flat` over the ranks from the current stream -> the work handle (None without data parallelism)."""
        if not self.dp:
            return None
        if self.measure_comm and self.comm_probe_every > 0 and it % self.comm_probe_every == 0:
            # per-bucket attribution (bench.py): `ready` = the moment the issuing stream has the bucket final (one event record on a
            # stream that exists anyway).  The collective's own time comes from the events RCCL's process group brackets it with
            # on ITS stream (Work._get_duration, TORCH_NCCL_ENABLE_TIMING=1), read in comm_table once the work is complete.
            # (A first version recorded a `done` event behind handle.wait() on a probe stream of its own: the extra stream moved
            # the round-robin assignment of the iteration's streams to hardware queues -- 756 -> 513 it/s on the one-rank RCCL path,
            # whether every iteration was probed or every fourth.  No new stream here.)
            ready = torch.cuda.Event(enable_timing=True)
            ready.record()
            handle = self._issue(flat)
            self._bucket_events.append((it, name, flat.numel() * 4, ready, handle))
            return handle
        return self._issue(flat)

    def _issue(self, flat):
        gbs = _fake_comm_gbs()
        if gbs is None:
            return torch.distributed.all_reduce(flat, group=self.group, async_op=True)
        # PRICED REHEARSAL (R3DG_DP_FAKE_COMM_GBS=<bus GB/s>, one-rank groups only): the identity collective, then a spin of
        # the time a ring all-reduce of this bucket takes over `world_assumed` ranks at that bus bandwidth --
        # 2 (W - 1) / W x bytes / B -- on ONE communication stream, so that the buckets serialise like RCCL's kernels do.
        # The returned handle's wait() makes the current stream wait for the end of the spin.
        W = int(os.environ.get("R3DG_DP_FAKE_COMM_WORLD", "8"))
        us = 2.0 * (W - 1) / W * flat.numel() * 4 / (gbs * 1e9) * 1e6
        comm = shared_stream(self.dev, "fake_comm")
        _lib.stream_wait(comm, torch.cuda.current_stream())
        if os.environ.get("R3DG_DP_FAKE_COMM_WITH_RCCL", "0") != "0":
            with torch.cuda.stream(comm):              # (the identity collective too: its launch + two stream joins)
                torch.distributed.all_reduce(flat, group=self.group, async_op=True).wait()
        begin = torch.cuda.Event(enable_timing=True) if self.measure_comm else None
        if begin is not None:
            begin.record(comm)
        _lib.check(_lib.lib().r3dg_spin(comm.cuda_stream, float(us)), "spin")
        done = torch.cuda.Event(enable_timing=self.measure_comm)
        done.record(comm)
        return _FakeCommHandle(done, begin)

    def wait(self, handle, name, it, side=None):
        """Make the current stream wait for a bucket's all-reduce; with `measure_comm` the wait is bracketed by events so that
        the time the stream actually stalls on it (the EXPOSED communication) can be read back (exposed_comm_ms).  `side`: the
        wait sits on this side stream (bucket A: under the shading backward), not on the compute stream -- it is then only
        recorded for comm_table's `released_us`, not counted as exposed."""
        if not self.measure_comm:
            handle.wait()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        handle.wait()
        e1.record()
        self._comm_events.append((it, e0, e1, name, side is not None))

    def exposed_comm_ms(self, split=False):
        """Mean per iteration of the time the compute stream waited for gradient all-reduces since measure_comm was set
        (synchronises).  The early bucket A is waited for on a side stream and is not part of it by construction.
        `split`: -> (total, {bucket name: mean ms per iteration})."""
        if not self._comm_events:
            return (None, {}) if split else None
        torch.cuda.synchronize(self.dev)
        per_iter, per_name = {}, {}
        self._released = {}
        for it, e0, e1, name, on_side in self._comm_events:
            self._released[(it, name)] = e1
            if on_side:
                continue
            ms = e0.elapsed_time(e1)
            per_iter[it] = per_iter.get(it, 0.0) + ms
            per_name[name] = per_name.get(name, 0.0) + ms
        self._comm_events = []
        n = max(1, len(per_iter))
        total = sum(per_iter.values()) / n
        return (total, {k: v / n for k, v in per_name.items()}) if split else total

    def comm_table(self, world_assumed=None):
        """Per-bucket attribution of the gradient all-reduces of the probed iterations since measure_comm was set (call after
        exposed_comm_ms; synchronises): for each bucket its bytes, when it became final on the stream that issued it (`ready_us`,
        relative to the first bucket of its iteration), when its first consumer's stream got past the wait (`released_us`), the
        collective's OWN time `collective_ms` -- bracketed by the events the process group records on RCCL's stream
        (Work._get_duration; needs TORCH_NCCL_ENABLE_TIMING=1 before the group is created, bench.py sets it); for a backend without
        them (gloo: the tests) the ready -> released interval, an upper bound -- and the bus bandwidth that time amounts to for a
        ring all-reduce over the group's ranks, 2 (W-1)/W x bytes / collective_ms.  Means over the probed iterations; None when
        nothing was probed."""
        if not self._bucket_events:
            return None
        torch.cuda.synchronize(self.dev)
        W = world_assumed or (int(os.environ.get("R3DG_DP_FAKE_COMM_WORLD", "8")) if _fake_comm_gbs() is not None else self.world)
        base_of, acc = {}, {}
        for it, name, nbytes, ready, handle in self._bucket_events:
            base = base_of.setdefault(it, ready)
            a = acc.setdefault(name, dict(bytes=nbytes, n=0, ready=0.0, released=0.0, n_rel=0, coll=0.0, timed_by=None))
            a["n"] += 1
            a["ready"] += base.elapsed_time(ready)
            rel = self._released.get((it, name))
            if rel is not None:
                a["released"] += base.elapsed_time(rel)
                a["n_rel"] += 1
            try:
                ms, by = float(handle._get_duration()), "collective's own events"
            except Exception:
                ms, by = (ready.elapsed_time(rel) if rel is not None else 0.0), "ready -> released (upper bound)"
            a["coll"] += ms
            a["timed_by"] = by
        self._bucket_events = []
        self._released = {}
        out = {}
        for name, a in acc.items():
            n = a["n"]
            coll = a["coll"] / n
            out[name] = dict(MB=round(a["bytes"] / 1e6, 2), ready_us=round(1e3 * a["ready"] / n, 1),
                             released_us=None if not a["n_rel"] else round(1e3 * a["released"] / a["n_rel"], 1),
                             collective_ms=round(coll, 4), timed_by=a["timed_by"],
                             bus_GBs=None if coll <= 0 or W < 2 else round(2.0 * (W - 1) / W * a["bytes"] / (coll * 1e-3) / 1e9, 1),
                             alg_GBs=None if coll <= 0 else round(a["bytes"] / (coll * 1e-3) / 1e9, 1), probed_iterations=n)
        return out
