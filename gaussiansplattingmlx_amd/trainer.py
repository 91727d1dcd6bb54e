"""Host-side mirror of the reference trainer's per-iteration path (Trainer/GaussianTrainer.swift:958-1086):
lossFn (render + L1/DSSIM loss) -> valueAndGrad -> per-tensor-LR Adam, over the C ABI.

Adds what the reference lacks: a data-parallel step.  Each rank renders its own view; parameter gradients are
summed over ranks (RCCL over xGMI via torch.distributed) and Adam runs identically on every rank with
grad_scale = 1/world_size (loss = mean over the views of the step).  Two exchanges:

  "allreduce"      one all-reduce over the whole flat gradient arena (N * (11 + 3K) floats);
  "sh_compressed"  the SH gradient of a view is rank-1 per Gaussian (basis_k(xyz - cam) x colorCot[3]), so ranks
                   all-gather colorCot (3 floats / Gaussian / view) plus all-reduce the 11 geometry floats, and each
                   rank rebuilds the summed SH gradient locally: at K = 25 and 8 ranks, 35 floats per Gaussian on
                   the wire instead of 86, and the all-reduce (2x traffic) shrinks to 11.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._lib import GS_ERR_REPLICA_MISMATCH, GsplatError
from .renderer import GaussianRenderer, _p

GS_ERR_WORKSPACE_OVERFLOW = 3
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-15      # the project's Adam (no bias correction): every step of this file

PARAM_ORDER = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")   # GaussianModel.swift:46-55
# arena layout: the 11 geometry floats per Gaussian first (one contiguous all-reduce), the SH tensors behind them
ARENA_ORDER = ("xyz", "scales", "rotation", "opacity", "features_dc", "features_rest")


def getLearningRates(current: int, total: int):
    """GaussianModel.swift:56-65."""
    return [0.00016 * max(1.0 - float(current) / float(total), 0.01), 0.0025, 0.0025 / 20, 0.005, 0.001, 0.025]


def arenaLearningRates(current: int, total: int):
    """getLearningRates permuted from PARAM_ORDER into ARENA_ORDER."""
    lr = dict(zip(PARAM_ORDER, getLearningRates(current, total)))
    return [lr[k] for k in ARENA_ORDER]


def exposureLearningRate(current: int, total: int, lr=(0.01, 0.001)) -> float:
    """The exposure's learning rate at step `current` of `total`: log-linear from lr[0] to lr[1], held at lr[1] from `total`
    on -- Inria's schedule for its per-image exposures (get_expon_lr_func, no delay)."""
    s = min(float(current) / float(total), 1.0) if total > 0 else 1.0
    return math.exp((1.0 - s) * math.log(lr[0]) + s * math.log(lr[1]))


def bilateralGridLearningRate(current: int, total: int, lr: float = 2e-3) -> float:
    """The bilateral grids' learning rate at step `current` of `total`: a linear warm-up from 1 % of lr over the first 1000
    steps, times an exponential decay to 1 % at `total` (held from there on) -- gsplat's schedule for its bilateral grids."""
    s = min(float(current) / float(total), 1.0) if total > 0 else 1.0
    return lr * (0.01 + 0.99 * min(current, 1000) / 1000.0) * 0.01 ** s


def view_for(step: int, rank: int, world: int, n_views: int) -> int:
    """View sharding: at step s the job consumes views [s*world, (s+1)*world) of a shared permutation; rank r takes
    the r-th of them.  No data-path collective is needed for the forward/backward; only gradients are exchanged."""
    return (step * world + rank) % n_views


def balanced_view_order(costs):
    """A visiting order of the views in which any `world` consecutive ones cost about the same.  A data-parallel step takes
    as long as its SLOWEST rank's view; with the views dealt in index order the eight views of a step are eight independent
    draws of the cost distribution (on the bench scene +-5 % around the mean: the maximum of eight is ~6 % above it, paid
    every step).  Sorted by cost and laid out as a zigzag -- ranks 0, 2, 4 ... of the sorted list going up, then ... 5, 3, 1
    coming down -- every window of consecutive views, cyclically, holds neighbours of the sorted list.  Every view is still
    visited once per pass; only the order changes (the reference draws its view at random every iteration,
    GaussianTrainer.swift:486-498, so no order is prescribed).  costs: one number per view (e.g. the view's traversed
    block-entries); returns a permutation of range(len(costs))."""
    order = sorted(range(len(costs)), key=lambda v: (costs[v], v))
    return order[0::2] + order[1::2][::-1]


def cc_block_floats(N: int) -> int:
    """Floats of one rank's block of the colour-cotangent all-gather (gs_dp_cc_floats): its [N,3] cotangents, then ONE word --
    the rank's overflow flag of the step as 0.0 / 1.0 --, padded to a multiple of four floats."""
    return (3 * int(N) + 1 + 3) & ~3


def exchange_sh_compressed(grad_geom: torch.Tensor, cc_local: torch.Tensor, cc_all: torch.Tensor, process_group=None):
    """The two collectives of the sh_compressed exchange: all-gather every rank's block (cc_block_floats: its colour
    cotangents [N,3] and, behind them, its word of the step's gate) -> [R, block] and sum the geometry slice of the gradient
    arena.  The caller then rebuilds the SH gradients (renderer.shGradFromViews), whose kernel ORs the gathered words into the
    step's gate (gathered_gate is the same thing in torch).  Round 5: the gate has no collective of its own any more."""
    import torch.distributed as dist
    dist.all_gather_into_tensor(cc_all.view(-1), cc_local.view(-1), group=process_group)   # flat: every backend takes it
    dist.all_reduce(grad_geom, op=dist.ReduceOp.SUM, group=process_group)


def gathered_gate(cc_all: torch.Tensor, N: int) -> bool:
    """The step's gate from the gathered blocks [R, cc_block_floats(N)]: was any rank's word raised?  What
    sh_grad_from_views_kernel computes on the device (csrc/projection.hip, adam_gate_word); here for hosts / tests in torch."""
    return bool((cc_all.view(cc_all.shape[0], -1)[:, 3 * int(N)] != 0).any().item())


def allreduce_gradients(grad_arena: torch.Tensor, process_group=None) -> float:
    """Sum the flat gradient arena over ranks (one collective for all six tensors; with the step's gate word riding as one
    more float behind the arena -- 0.0 / 1.0 per rank, so the sum is non-zero on every rank iff some rank's forward
    overflowed -- when the caller passes arena + word).  Returns the scale Adam must apply (1/world) so that the step uses
    the mean over the step's views."""
    import torch.distributed as dist
    world = dist.get_world_size(process_group)
    if world > 1:
        dist.all_reduce(grad_arena, op=dist.ReduceOp.SUM, group=process_group)
    return 1.0 / world


class ReplicaMismatch(GsplatError):
    """check_replicas / gs_dp_check_replicas: the ranks of a data-parallel job do not hold the same model."""

    def __init__(self, msg):
        super().__init__(GS_ERR_REPLICA_MISMATCH, msg)


def check_replicas(N: int, arena: torch.Tensor, process_group=None, rank: int | None = None):
    """"verify with an all-reduce'd checksum every densify step".  Densification is replicated without
    communication (same classify inputs, same noise seed: GaussianTrainer.swift:766-908); a rank whose model diverged would
    hang the job in the next size-dependent collective.  One fixed-size collective: (N, sum of the arena in f64, sum of its
    magnitudes) and their negatives, max-reduced -- maxima and minima in one call.  Raises ReplicaMismatch on EVERY rank (the
    verdict is built from reduced values) unless all three agree.  The torch form of gs_dp_check_replicas."""
    import torch.distributed as dist
    w = torch.stack([torch.tensor(float(N), dtype=torch.float64, device=arena.device), arena.sum(dtype=torch.float64),
                     arena.abs().sum(dtype=torch.float64)])
    mine = [float(x) for x in w.cpu()]
    both = torch.cat([w, -w])
    dist.all_reduce(both, op=dist.ReduceOp.MAX, group=process_group)
    hi, lo = [float(x) for x in both[:3].cpu()], [-float(x) for x in both[3:].cpu()]
    if hi == lo:
        return
    _raise_replica_mismatch(hi, lo, mine, dist.get_rank(process_group) if rank is None else rank)


PLAN_WORDS = ("N_new", "applies", "total", "keep", "split", "clone", "prune", "N")      # gs_densify_plan_read's order


def check_plans(words, process_group=None, device=None, side_stream=None, rank: int | None = None):
    """Round 6: the ranks' densify PLANS (gs_densify_plan_read's eight words) compared in one fixed-size collective -- (w, -w)
    max-reduced: maxima and minima in one call.  On a GPU it runs on side_stream, which does not wait for the current stream's
    queue: the event's gather keeps the device busy while the ranks agree.  Raises ReplicaMismatch on EVERY rank (the verdict is
    built from reduced values) unless all words agree: a rank that planned another N would otherwise hang the job in the next
    size-dependent collective.  The torch form of gs_dp_check_plan."""
    import torch.distributed as dist
    w = torch.tensor([float(x) for x in words], dtype=torch.float64)
    both = torch.cat([w, -w])
    if device is not None and torch.device(device).type == "cuda":
        ctx = torch.cuda.stream(side_stream) if side_stream is not None else torch.cuda.stream(torch.cuda.current_stream(device))
        with ctx:
            dev = both.to(device, non_blocking=False)
            dist.all_reduce(dev, op=dist.ReduceOp.MAX, group=process_group)
            both = dev.cpu()
    else:
        dist.all_reduce(both, op=dist.ReduceOp.MAX, group=process_group)
    n = len(words)
    hi, lo = [float(x) for x in both[:n]], [-float(x) for x in both[n:]]
    if hi == lo:
        return
    diff = " ".join(f"{name} in [{l:.0f}, {h:.0f}]" for name, h, l in zip(PLAN_WORDS, hi, lo) if h != l)
    raise ReplicaMismatch(f"the ranks planned different densify events ({diff}); rank "
                          f"{dist.get_rank(process_group) if rank is None else rank} planned new N = {int(words[0])} from N = {int(words[-1])}")


def check_replicas_begin(N: int, arena: torch.Tensor, process_group=None):
    """check_replicas queued: the checksum and its max all-reduce are enqueued, nothing is read back (check_replicas_end
    does that).  Returns the pending state."""
    import torch.distributed as dist
    w = torch.stack([torch.tensor(float(N), dtype=torch.float64, device=arena.device), arena.sum(dtype=torch.float64),
                     arena.abs().sum(dtype=torch.float64)])
    both = torch.cat([w, -w])
    work = dist.all_reduce(both, op=dist.ReduceOp.MAX, group=process_group, async_op=True)
    return (w, both, work)


def check_replicas_end(pending, process_group=None, rank: int | None = None):
    import torch.distributed as dist
    w, both, work = pending
    work.wait()
    mine = [float(x) for x in w.cpu()]
    hi, lo = [float(x) for x in both[:3].cpu()], [-float(x) for x in both[3:].cpu()]
    if hi == lo:
        return
    _raise_replica_mismatch(hi, lo, mine, dist.get_rank(process_group) if rank is None else rank)


def _raise_replica_mismatch(hi, lo, mine, rank):
    names = ("N", "sum", "magnitudes")
    diff = " ".join(n for n, h, l in zip(names, hi, lo) if h != l)
    raise ReplicaMismatch(f"the ranks hold different models ({diff}): over the ranks N in [{lo[0]:.0f}, {hi[0]:.0f}], sum in "
                          f"[{lo[1]!r}, {hi[1]!r}], sum of magnitudes in [{lo[2]!r}, {hi[2]!r}]; rank {rank} has N = {mine[0]:.0f}, "
                          f"sum = {mine[1]!r}, sum of magnitudes = {mine[2]!r}")


def exchange_summary(dp_impl, dp_exchange, world, N, geom_numel, numel, steps, sums, counts, rccl_version, source, views_per_rank=1):
    """The `exchange` block of a data-parallel bench line from what a timed run accumulated.  sums: milliseconds summed over
    the timed steps -- "gather" / "reduce" = duration of the colour-cotangent all-gather and the gradient all-reduce on the
    communication stream (they include the wait for the slowest peer; "gate": rounds 3-4's 4-byte all-reduce, gone in round 5 --
    its count is 0 and gate_ms null); "exposed_gather" /
    "exposed_reduce" = time the render stream stood waiting for them, i.e. wire time NOT hidden under compute.  counts: how
    many steps contributed a duration per collective (0: the backend keeps none -> null).  Bytes are per rank and step:
    what the rank hands to the collective (out) and what it holds afterwards (in)."""
    n = max(int(steps), 1)
    per = lambda k: round(sums[k] / counts[k], 4) if counts.get(k) else None
    xg, xr = sums["exposed_gather"] / n, sums["exposed_reduce"] / n
    out = dict(dp_impl=dp_impl, dp_exchange=dp_exchange, world=int(world), steps_measured=int(steps), rccl_version=rccl_version,
               timing_source=source, gate_ms=per("gate"), gather_ms=per("gather"), reduce_ms=per("reduce"),
               exposed_gather_ms=round(xg, 4), exposed_reduce_ms=round(xr, 4), exposed_ms=round(xg + xr, 4))
    # round 5: the gate word rides in the step's first payload (behind the colour cotangents / behind the gradient arena)
    if dp_exchange == "sh_compressed":
        blk = 4 * cc_block_floats(N) * int(views_per_rank)        # (a rank's views' blocks one behind the other)
        out.update(gather_bytes_out=blk, gather_bytes_in=blk * int(world), reduce_bytes=4 * int(geom_numel),
                   collectives_per_step=2, gate_rides_in="gather", views_per_rank=int(views_per_rank))
    else:
        out.update(gather_bytes_out=0, gather_bytes_in=0, reduce_bytes=4 * (int(numel) + 1), collectives_per_step=1,
                   gate_rides_in="reduce")
    out["gate_bytes"] = 4
    return out


class GaussModel:
    """Six raw parameter tensors as views into one flat f32 arena (so one all-reduce / one Adam launch covers them).

    Every tensor starts on a 16-byte boundary of the arena (its segment is padded to a multiple of four floats; the pad
    stays zero in all four arenas): the fused kernels address the SH rows as float4 and keep them in registers between
    the staging load and the Adam update only then, and an odd Gaussian count after a densify event used to put them
    on the slower unaligned path.

    The arena is a prefix of a buffer with room for `capacity` Gaussians, and the parameters are double-buffered, so
    a densify / prune event gathers straight into the other buffer and flips -- no allocation, no copy -- as long as
    the new count fits (it regrows by 1.5x otherwise).

    `stride` (round 5): the rows every tensor's segment has room for.  stride = N is the packed layout above (what a
    data-parallel all-reduce of the leading geometry slice wants).  The trainer's planned densify event lays the new
    model out at stride = capacity instead: the six tensors' POINTERS then do not depend on the new count, which is still
    on the device when the gather is queued (split_and_prune); the rows between N and the stride are never read (every
    kernel of the path indexes by Gaussian), numel / seg_end describe the strided arena."""

    def __init__(self, params: dict, device, capacity: int | None = None):
        self.device = device
        self._row = {k: tuple(params[k].shape[1:]) for k in ARENA_ORDER}
        self._per = {k: int(np.prod(self._row[k])) if len(self._row[k]) else 1 for k in ARENA_ORDER}
        self.floats_per_gaussian = int(sum(self._per.values()))
        self.K = self._row["features_rest"][0] + 1
        N = int(params["xyz"].shape[0])
        self._pbuf = [None, None]
        self._cur = 0
        self._gbuf = self._mbuf = self._vbuf = None
        self._mspare = self._vspare = None      # the moments' staging (stagingMoments): allocated by the first event that keeps them
        self._staged = None
        self.stride = N
        self._layout(N, max(int(capacity or N), N))
        for k in ARENA_ORDER:
            src = params[k]
            if not isinstance(src, torch.Tensor):
                src = torch.as_tensor(np.ascontiguousarray(src, np.float32))
            self._views[k].copy_(src.reshape(self._views[k].shape))

    def _buf(self, old, floats, zero=False):
        if old is not None and old.numel() >= floats + 4:
            return old
        # (+ 4: one spare word behind every arena -- a data-parallel all-reduce carries the step's gate there)
        return (torch.zeros if zero else torch.empty)(max(floats, 4) + 4, dtype=torch.float32, device=self.device)

    def _offsets(self, N: int):
        """(start of every tensor's segment, total floats) for N Gaussians: segments padded to multiples of 4 floats."""
        starts, off = [], 0
        for k in ARENA_ORDER:
            starts.append(off)
            off += (N * self._per[k] + 3) & ~3
        return starts, off

    def _zero_pads(self, buf, N):
        """The up to three pad floats behind every tensor (a reused buffer may hold an older layout's values there)."""
        starts, total = self._offsets(N)
        for k, off, nxt in zip(ARENA_ORDER, starts, starts[1:] + [total]):
            if off + N * self._per[k] < nxt:
                buf[off + N * self._per[k]:nxt].zero_()

    def _carve(self, buf, N, stride=None):
        views = {}
        starts, _ = self._offsets(N if stride is None else stride)
        for k, off in zip(ARENA_ORDER, starts):
            n = N * self._per[k]
            views[k] = buf[off:off + n].view((N,) + self._row[k])
        return views

    def _layout(self, N: int, capacity: int, pads=("arena", "grad", "m", "v"), stride=None):
        stride = N if stride is None else int(stride)
        floats = self._offsets(max(capacity, stride))[1]
        self.capacity = capacity
        self.N = N
        self.stride = stride
        starts, self.numel = self._offsets(stride)
        self.seg_start = np.asarray(starts, np.int64)
        self.seg_end = np.asarray(starts[1:] + [self.numel], np.int64)      # a segment's pad takes its learning rate (and stays 0)
        self.geom_numel = int(self.seg_end[3])     # xyz + scales + rotation + opacity
        self._pbuf[self._cur] = self._buf(self._pbuf[self._cur], floats, zero=True)
        self._gbuf, self._mbuf, self._vbuf = (self._buf(b, floats, zero=True) for b in (self._gbuf, self._mbuf, self._vbuf))
        self.arena = self._pbuf[self._cur][:self.numel]
        self.grad, self.m, self.v = self._gbuf[:self.numel], self._mbuf[:self.numel], self._vbuf[:self.numel]
        if stride == N:
            for name in pads:  # (each pad is a tiny launch of its own: a caller that zeroes a whole arena anyway leaves it out)
                self._zero_pads(getattr(self, name), N)
        self._views, self._gviews = self._carve(self.arena, N, stride), self._carve(self.grad, N, stride)

    def getParams(self):
        return self._views

    def getGrads(self):
        return self._gviews

    def stagingViews(self, N_new: int, stride=None) -> dict:
        """Views for N_new Gaussians in the OTHER parameter buffer (the densify gather writes them).  stride: rows per
        tensor segment of the staged layout (default: packed, N_new)."""
        cap = self.capacity if N_new <= self.capacity else int(N_new * 1.5)
        stride = N_new if stride is None else int(stride)
        other = 1 - self._cur
        # (zeroed once, when it is allocated: a capacity-strided layout spans rows between N and the stride that no kernel
        # writes, and a consumer that reads `arena` whole -- a checksum, isfinite, a clone -- would meet uninitialised floats)
        self._pbuf[other] = self._buf(self._pbuf[other], self._offsets(max(cap, stride))[1], zero=True)
        self._staged = (N_new, cap, stride)
        return self._carve(self._pbuf[other][:self._offsets(stride)[1]], N_new, stride)

    def stagingBase(self, capacity: int):
        """The OTHER parameter buffer as one flat tensor with room for `capacity` Gaussians in the packed layout (the packed
        planned gather lays the tensors out itself, on the device, once the new count is known there); commitStaged(N_new)
        then flips to it in the packed layout for N_new."""
        cap = max(int(capacity), self.capacity)
        other = 1 - self._cur
        self._pbuf[other] = self._buf(self._pbuf[other], self._offsets(cap)[1], zero=True)
        self._staged = (None, cap, None)
        return self._pbuf[other]

    def getMoments(self):
        """(m, v): the two Adam moment arenas as views keyed like the parameters."""
        return self._carve(self.m, self.N, self.stride), self._carve(self.v, self.N, self.stride)

    def stagingMoments(self):
        """(m, v) views for the rows stagingViews has just staged (packed layout), in spare moment buffers: an event that
        keeps the Adam state gathers the moments into them (strategy="adc"), and commitStaged(moments=True) flips to them."""
        N_new, cap, stride = self._staged
        if N_new is None or stride != N_new:
            raise ValueError("stagingMoments: after stagingViews(N_new) in the packed layout")
        floats = self._offsets(max(cap, stride))[1]
        self._mspare, self._vspare = self._buf(self._mspare, floats, zero=True), self._buf(self._vspare, floats, zero=True)
        n = self._offsets(stride)[1]
        return self._carve(self._mspare[:n], N_new, stride), self._carve(self._vspare[:n], N_new, stride)

    def commitStaged(self, N_new=None, zero=True, moments=False):
        """Flip to the staged buffer (split_and_prune phase 6, GaussianTrainer.swift:900-905); gradients and Adam
        moments are zeroed (the reference re-creates the optimizer state, :1104-1109).  N_new: the row count when it was
        not known at staging time (the planned event stages `capacity` rows' worth of pointers); zero=False: the caller
        has zeroed the buffers whole already.  moments=True: flip to the moments staged by stagingMoments as well (they are
        then kept, whatever `zero` says; the gradients are zeroed)."""
        n_staged, cap, stride = self._staged
        N_new = n_staged if N_new is None else int(N_new)
        self._staged = None
        self._cur = 1 - self._cur
        if moments:
            self._mbuf, self._mspare = self._mspare, self._mbuf
            self._vbuf, self._vspare = self._vspare, self._vbuf
            self._layout(N_new, cap, pads=("arena", "m", "v"))
            self.grad.zero_()
            return
        self._layout(N_new, cap, pads=("arena",), stride=None if stride is None or (stride == n_staged and N_new == n_staged) else stride)
        if zero:
            self.grad.zero_()                          # gradients and moments are zeroed whole, pads included
            self.resetOptimizerState()

    def zeroOptimizerBuffers(self, grads: bool = False):
        """The moment buffers (and the gradient buffer) zeroed WHOLE -- whatever layout comes next."""
        self._mbuf.zero_()
        self._vbuf.zero_()
        if grads:
            self._gbuf.zero_()

    def commit(self, params: dict):
        """Replace the six tensors by copies of `params` (any source)."""
        out = self.stagingViews(int(params["xyz"].shape[0]))
        for k in ARENA_ORDER:
            src = params[k]
            if not isinstance(src, torch.Tensor):
                src = torch.as_tensor(np.ascontiguousarray(src, np.float32))
            out[k].copy_(src.reshape(out[k].shape))
        self.commitStaged()

    def resetOptimizerState(self):
        self.m.zero_()
        self.v.zero_()

    def restride(self, capacity: int):
        """Lays the model out at stride = capacity >= N rows per tensor segment in fresh buffers, parameters and moments kept:
        rows can then be appended in place up to `capacity` (setCount) with no pointer moving (the MCMC strategy's growth)."""
        capacity = max(int(capacity), self.N)
        if self.stride == capacity and self.capacity == capacity:
            return
        old = {name: self._carve(getattr(self, name), self.N, self.stride) for name in ("arena", "m", "v")}
        self._pbuf[self._cur] = self._gbuf = self._mbuf = self._vbuf = None
        self._pbuf[1 - self._cur] = None
        self._layout(self.N, capacity, stride=capacity)
        for name in ("arena", "m", "v"):
            new = self._carve(getattr(self, name), self.N, self.stride)
            for k in ARENA_ORDER:
                new[k].copy_(old[name][k])

    def setCount(self, N: int):
        """The count after rows were appended in place at the current stride (N <= stride): the views are carved anew."""
        if not self.N <= int(N) <= self.stride:
            raise ValueError(f"setCount: {N} is not in [{self.N}, {self.stride}]")
        self._layout(int(N), self.capacity, pads=(), stride=self.stride)


def _adamStep(r, fn: str, n, tensors, seg_end, lrs, scale, before=(), after=()):
    """One of the library's Adam kernels (fn: gs_adam_step, gs_adam_step_add, gs_adam_step_visible) with the project's Adam:
    beta (0.9, 0.999), eps 1e-15, no bias correction.  tensors = (parameters, gradients, m, v) over n floats; seg_end / lrs: the
    segments' ends (a ctypes array as it is, or a sequence) and learning rates; scale: grad_scale.  before / after: what fn
    takes in front of the constants (gs_adam_step_visible's row widths) and behind grad_scale."""
    k = len(lrs)
    ends = seg_end if isinstance(seg_end, C.Array) else (C.c_longlong * k)(*[int(x) for x in seg_end])
    r._check(getattr(r.lib, fn)(r.ctx, n, *[_p(t) for t in tensors], k, ends, (C.c_float * k)(*lrs), *before,
                                C.c_float(ADAM_BETA1), C.c_float(ADAM_BETA2), C.c_float(ADAM_EPS), C.c_float(scale), *after))


def _set_adc_stats(r, stats):
    # (a step sets the statistic in _beginIteration, and behind densify_until no step does: then nothing is put back either)
    if r.adcStats is not stats:
        r.setADCStats(*(stats or (None, None, None)))


class _Borrowed:
    """The caller's renderer, lent to the trainer for one call: `with _Borrowed(r, *keep) as lent` reads the settings named in
    `keep` through the renderer's getters, lent.set(name=value, ...) reads a setting that is not held yet and then sets it, and
    on the way out, whatever happened, everything held is put back in SETTINGS' order and the `unbind` per-view tables are
    unbound (a step binds its view's rows itself; they are the trainer's, so there is nothing of the caller's to put back)."""
    SETTINGS = {       # name: (read, write)
        "depth_gradient": (lambda r: r.getTuning("depth_gradient"), lambda r, v: r.setTuning(depth_gradient=v)),
        "host_overflow_errors": (lambda r: r.getTuning("host_overflow_errors"), lambda r, v: r.setTuning(host_overflow_errors=v)),
        "mcmc": (lambda r: r.mcmc, lambda r, v: r.setMCMC(v)),
        "sh_degree": (lambda r: r.shDegree, lambda r, v: r.setSHDegree(v)),
        "filter_3d": (lambda r: r.filter3D, lambda r, v: r.setFilter3D(v)),
        "sparse_adam": (lambda r: r.sparseAdam, lambda r, v: r.setSparseAdam(v)),
        "adc_stats": (lambda r: r.adcStats, _set_adc_stats),
        "background": (lambda r: r.customBackground, lambda r, v: r.setBackground(v)),
        "loss_mask": (lambda r: r.lossMask, lambda r, v: r.setLossMask(v)),
        "pose": (lambda r: r.poseCorrection, lambda r, v: r.setPoseCorrection(*v)),
    }

    def __init__(self, r, *keep, unbind=()):
        self.r, self.unbind = r, unbind
        self.was = {name: self.SETTINGS[name][0](r) for name in keep}

    def set(self, **settings):
        for name, value in settings.items():
            read, write = self.SETTINGS[name]
            if name not in self.was:
                self.was[name] = read(self.r)
            write(self.r, value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for name, (_, write) in self.SETTINGS.items():
            if name in self.was:
                write(self.r, self.was[name])
        for t in self.unbind:
            t.unbind(self.r)
        return False


class _PerViewTable:
    """The trainable state of one per-view correction (pose_opt, exposure_opt, bilateral_grid): for each of n_views training
    views a row of `width` floats and its two Adam moments, the gradient the step writes, and how a row is bound to the renderer.
    Rows lie a multiple of four floats apart: gs_adam_step takes 16-byte aligned arenas.

    feature: the trainer's keyword, in front of every message.  start: a row's first value (None: zero).  segments / rates:
    gs_adam_step's segment ends within a row and a callable (iteration, iterationCount) -> their learning rates.
    bind(renderer, row, grad) binds a view's row and its gradient for a step, bind(renderer, None, None) unbinds.  shared_grad:
    one gradient row serves every view (only the visited view's is ever read) where a row per view would be memory for nothing."""

    def __init__(self, feature, n_views, width, device, segments, rates, bind, start=None, shared_grad=False):
        self.feature, self.nViews, self.width = feature, int(n_views), int(width)
        self.segments, self.rates, self.bind = tuple(segments), rates, bind
        z = lambda n: torch.zeros((n, (self.width + 3) & ~3), dtype=torch.float32, device=device)[:, :self.width]   # noqa: E731
        self.rows, self.m, self.v = z(self.nViews), z(self.nViews), z(self.nViews)
        self.grad = z(1 if shared_grad else self.nViews)
        if start is not None:
            self.rows.copy_(start)

    def row(self, viewKey) -> int:
        if viewKey is None or isinstance(viewKey, (list, tuple)):
            raise ValueError(f"{self.feature}: every trainStep needs the viewKey of its one view")
        row = int(viewKey)
        if row != viewKey or not 0 <= row < self.nViews:
            raise ValueError(f"{self.feature}: viewKey {viewKey!r} is not one of 0 .. {self.nViews - 1}")
        return row

    def gradRow(self, row: int):
        return self.grad[row % self.grad.shape[0]]

    def bindRow(self, renderer, row: int):
        """The view's row, for every forward and loss of this step (repeats included) and their backward."""
        self.bind(renderer, self.rows[row], self.gradRow(row))

    def unbind(self, renderer):
        self.bind(renderer, None, None)

    def adam(self, renderer, row: int, iteration: int, iterationCount: int):
        """Adam on the view's row (gs_adam_step; the project's Adam: beta (0.9, 0.999), eps 1e-15, no bias correction): gated like
        the step's other optimizer kernels, so a step from a blank render moves no row either.  The other views' rows and moments
        are left alone."""
        _adamStep(renderer, "gs_adam_step", self.width, (self.rows[row], self.gradRow(row), self.m[row], self.v[row]),
                  self.segments, self.rates(iteration, iterationCount), 1.0)


def _require_single_device(feature, views_per_rank, process_group, dp_bootstrap, exchange_impl, n_views=1):
    """What the MCMC strategy and every per-view correction ask of the trainer's arguments: one view per step, on one device --
    and, of a per-view correction, n_views (strategy='mcmc' has no use for it and leaves the default)."""
    if views_per_rank != 1:
        raise ValueError(f"{feature}: one view per step only (views_per_rank > 1 is not supported)")
    if process_group is not None or dp_bootstrap is not None or exchange_impl == "native":
        raise ValueError(f"{feature}: single-device steps only (no process group, dp_bootstrap or native exchange)")
    if n_views is None or isinstance(n_views, bool) or int(n_views) != n_views or int(n_views) < 1:
        raise ValueError(f"{feature} needs n_views >= 1 (view keys 0 .. n_views - 1)")


# The trainer's optional features in the order the constructor checks them (DESIGN.md section 32 has the table for readers):
#   keyword: (its config class as (module, "a Class") -- None for a plain switch --, the label in front of its single-device
#             messages, ((a switch it is refused with, the message), ...), are the refusals checked BEHIND the single-device
#             requirement?)
# Every enabled feature takes single-device steps with one view (_require_single_device).  The switches a refusal may name:
# the keywords, "mcmc" / "adc" for the strategies and "no_densify" for densify=False under the reference strategy.
_FEATURES = {
    "sh_schedule": ((".sh_schedule", "an SHDegreeSchedule"), "sh_schedule", (), False),
    "depth": ((".depth_loss", "a DepthConfig"), "depth", (), False),
    "normal": ((".normal_loss", "a NormalConfig"), "normal", (), False),
    "distortion": ((".distortion", "a DistortionConfig"), "distortion", (), False),
    "background": ((".background", "a BackgroundConfig"), "background", (), False),
    "sparse_adam": (None, "sparse_adam", (
        ("mcmc", "sparse_adam: the reference strategy only (strategy='mcmc' moves every Gaussian every step)"),
        ("filter_3d", "sparse_adam: not with filter_3d=True")), False),
    "adc": ((".adc", "an ADCConfig"), "strategy='adc'", (
        ("filter_3d", "strategy='adc': not with filter_3d"), ("contrib_prune", "strategy='adc': not with contrib_prune"),
        ("sparse_adam", "strategy='adc': not with sparse_adam")), True),
    "contrib_prune": ((".contrib_prune", "a ContribPruneConfig"), "contrib_prune", (
        ("mcmc", "contrib_prune: the reference strategy only (not with strategy='mcmc')"),), False),
    "absgrad": ((".absgrad", "an AbsGradConfig"), "absgrad", (
        ("mcmc", "absgrad: the reference strategy or strategy='adc' (not with strategy='mcmc')"),
        ("no_densify", "absgrad changes the densification criterion: not with densify=False")), False),
    "mcmc": ((".mcmc", "an MCMCConfig"), "strategy='mcmc'", (), False),
    "filter_3d": (None, "filter_3d", (("mcmc", "filter_3d: the reference strategy only (not with strategy='mcmc')"),), False),
    "pose_opt": (None, "pose_opt", (), False),
    "exposure_opt": (None, "exposure_opt", (), False),
    "bilateral_grid": (None, "bilateral_grid", (
        ("exposure_opt", "bilateral_grid and exposure_opt are exclusive (a constant grid is an exposure)"),), False),
}


def _admit(feature, value, on, where, n_views=1):
    """One enabled feature's checks from _FEATURES: its config's type and validate(), what it is refused with (on: switch ->
    is it on), the single-device requirement (where: views_per_rank, process_group, dp_bootstrap, exchange_impl).  Returns
    the value."""
    config, label, refusals, late = _FEATURES[feature]
    if config is not None:
        import importlib
        if not isinstance(value, getattr(importlib.import_module(config[0], __package__), config[1].split()[1])):
            raise ValueError(f"{feature} must be {config[1]}")
        value.validate()
    refused = [message for switch, message in refusals if on[switch]]
    if refused and not late:
        raise ValueError(refused[0])
    _require_single_device(label, *where, n_views)
    if refused:
        raise ValueError(refused[0])
    return value


class GaussianTrainer:
    def __init__(self, model: GaussModel, gaussRender: GaussianRenderer, iterationCount: int = 30000,
                 lambda_dssim: float = 0.2, process_group=None, dp_exchange: str = "sh_compressed",
                 exchange_when_single: bool = False, densify: bool = True, fuse_adam: bool = True,
                 exchange_impl: str = "torch", dp_bootstrap=None, views_per_rank: int = 1, pose_opt: bool = False,
                 pose_lr=(1e-4, 1e-4), n_views: int | None = None, strategy: str = "reference", mcmc=None,
                 exposure_opt: bool = False, exposure_lr=(0.01, 0.001), bilateral_grid: bool = False,
                 bilateral_grid_shape=(16, 16, 8), bilateral_grid_lr: float = 2e-3, bilateral_grid_tv: float = 10.0,
                 filter_3d: bool = False, filter_cameras=None, filter_3d_interval: int = 100, contrib_prune=None,
                 absgrad=None, sparse_adam: bool = False, background=None, depth=None, adc=None, sh_schedule=None, normal=None,
                 distortion=None):
        """exchange_impl: who issues the collectives of a data-parallel step.  "torch": torch.distributed on
        process_group (RCCL when its backend is nccl; gloo for CPU rehearsals).  "native": the library itself
        (gs_dp_step: RCCL on its own side stream, the same event ordering) -- process_group is then only used to hand
        rank 0's RCCL id to the others, or not at all when dp_bootstrap = (id_bytes, rank, world) is given.

        views_per_rank (round 6): V > 1 makes a step take V views on THIS rank -- one update from the mean loss over the
        world x V views of the step ("8 views/step is a semantic extension: loss = mean over views").  Each view
        runs forward + loss + the data-parallel backward exactly as a rank of a V-times larger job would (its colour-cotangent
        block with its gate word behind it, its geometry gradients, its |grad xyz| into the densify statistic); the blocks of
        the rank's views lie one behind the other in the buffer the all-gather hands over (without a process group that buffer
        IS the gathered one: the collective replaced by addressing), the geometry gradients are summed over the rank's views
        before the all-reduce, the SH rebuild runs over all world x V blocks and Adam at grad_scale 1 / (world x V).  With
        world = 1, V = 8 this is BASELINE config 4's arithmetic -- eight views, one update -- on one card.  sh_compressed
        exchange, torch issuer (or no group at all); world x V <= 16.

        pose_opt: per-view camera pose refinement (include/gsplat.h gs_set_pose_correction).  Every training view v has a
        correction delta_v = (w, tau) of its camera-to-world pose, c2w' = c2w [[R(w), tau], [0, 1]] in the camera's own frame,
        zero at the start and trained by the loss with its own Adam step (the project's Adam, no bias correction) at
        pose_lr = (rotation rate in radians, translation rate in scene units) -- each moves a component by about its rate per
        step (about three times that on a view's first steps: no bias correction); the defaults (1e-4, 1e-4) keep a correct
        camera within ~0.1 px of where it is at 800 px and a focal of ~1000, and reach a degree in a few hundred visits of a view.
        Raise them for poses known to be far off.  Needs
        n_views (the view keys are 0 .. n_views - 1) and a viewKey on every step; single-device steps only (one view per step,
        no process group, no native exchange).  Off (the default): no kernel, buffer or result differs.

        exposure_opt: per-view exposure compensation (include/gsplat.h gs_set_exposure).  Every training
        view v has an affine colour transform M_v = [A | b] (3 x 4, the identity at the start); the loss of a step is taken of
        A render + b, and M_v is trained with it by its own Adam step (the project's Adam: beta (0.9, 0.999), eps 1e-15, no bias
        correction) at exposureLearningRate(t, iterationCount, exposure_lr), log-linear from exposure_lr[0] to exposure_lr[1]
        (Inria's defaults 0.01 -> 0.001).  Only the visited view's row moves.  Needs n_views and a viewKey on every step, as
        pose_opt does; single-device steps only.  Composes with pose_opt, strategy='mcmc', an anti-aliased renderer and
        referenceParamReload (which restores the model, not the exposures).  exposures() returns the learned transforms,
        exposedRender(render, viewKey) a render under one.  Off (the default): no kernel, buffer or result differs.

        bilateral_grid: per-view bilateral grid colour correction (include/gsplat.h gs_set_bilateral_grid, DESIGN.md section
        13), exposure compensation that varies over the image and with the render's luminance.  Every training view v has a grid
        of bilateral_grid_shape = (grid_w, grid_h, grid_l) nodes, each a 3 x 4 affine transform (the identity at the start);
        the loss of a step is taken of the render under the view's grid, and the grid is trained with it (plus
        bilateral_grid_tv times its total variation) by its own Adam step (the project's Adam: beta (0.9, 0.999), eps 1e-15, no
        bias correction) at bilateralGridLearningRate(t, iterationCount, bilateral_grid_lr).  Only the visited view's grid moves
        and only it is regularised (gsplat regularises all grids every step).  Needs n_views and a viewKey on every step;
        single-device steps only; not together with exposure_opt.  Composes with pose_opt, strategy='mcmc', an anti-aliased
        renderer and referenceParamReload.  bilateralGrids() returns the learned grids, bilateralRender(render, viewKey) a render
        under one.  Off (the default): no kernel, buffer or result differs.

        strategy: "reference" (the default: the reference's densification -- clone / split by accumulated |grad xyz|, prune,
        optimizer reset every 100 steps -- when densify is on), "adc" (adaptive density control: the last paragraph) or "mcmc":
        the MCMC strategy (mcmc.MCMCConfig, include/gsplat.h
        gs_set_mcmc) with the settings `mcmc` (None: MCMCConfig()).  Every step adds the regularisers'
        gradients and, behind Adam, the position noise; behind steps refine_start < t < refine_stop, t % refine_every == 0, dead
        Gaussians are relocated onto live ones and the count grows by grow_rate up to cap_max.  The reference strategy is then
        off (densify is ignored).  The model is laid out at stride = capacity >= cap_max on construction, so growth appends in
        place; lastMCMCStats holds the last event's counts.  Single-device steps only (no process group, dp_bootstrap, native
        exchange or views_per_rank > 1, no referenceParamReload); composes with pose_opt and an anti-aliased renderer.

        filter_3d: Mip-Splatting's 3-D smoothing filter (include/gsplat.h gs_set_filter3d).  The trainer
        owns a [capacity] buffer of filter widths, computed from filter_cameras (the training cameras, as given: a pose_opt
        run does not move them) at construction, behind every committed densify event, behind every parameter reload and
        every filter_3d_interval iterations; every step renders and differentiates under it, and save_snapshot writes the
        BAKED parameters (gs_filter3d_bake), which any viewer renders as the filtered model.  Single-device steps and the
        reference strategy only; composes with pose_opt, exposure_opt, bilateral_grid, an anti-aliased renderer and
        referenceParamReload.  filter3D() returns the widths of the current model.  Off (the default): no kernel, buffer or
        result differs.

        contrib_prune: contribution-based pruning (contrib_prune.ContribPruneConfig, include/gsplat.h gs_render_contrib, DESIGN.md
        section 15).  Behind every iteration listed in contrib_prune.at -- after that iteration's split_and_prune, if it has one --
        the model is rendered from contrib_prune.cameras (under pose_opt from refinedCamera(i, cameras[i]): view keys 0 .. len - 1),
        every Gaussian is scored by the largest (score="max", RadSplat) or the summed (score="sum") blend weight T alpha it gets
        at any pixel of any of them, and those below contrib_prune.threshold are pruned through the densify event's own scan,
        output map and gather (the planned ones where plannedDensify).  The event commits as a committed densify event does:
        optimizer state and gradient accumulators reset, filter_3d widths recomputed, depth cuts kept (nothing gets longer).  An
        event that would prune everything prunes nothing.  lastContribPruneStats holds the last event's N, kept, pruned and
        threshold; pruneByContribution(cameras, threshold, score) runs the same event on demand (compaction before a snapshot).
        Single-device steps and the reference strategy only; composes with pose_opt, exposure_opt, bilateral_grid, filter_3d, an
        anti-aliased renderer and densify on or off.  Off (the default): no kernel, buffer or result differs.

        absgrad: AbsGS densification (absgrad.AbsGradConfig, include/gsplat.h gs_set_absgrad; Ye et al.
        2024, gsplat's absgrad=True).  The trainer turns the renderer's absgrad setting on: every step's blend backward also sums,
        per Gaussian, the per-pixel absolute values of the 2-D mean gradient, and xyzGradAccumulation gets hypot(W/2 Ax, H/2 Ay)
        in place of |grad xyz| -- a large Gaussian over fine detail, whose per-pixel gradients cancel in the signed sum, is then
        split.  gradientThreshold becomes absgrad.threshold; the global step denominator, classifyGaussians and the event code
        stay as they are: only what is summed changes.  The default threshold, 0.0008, is gsplat's documented value for absgrad,
        where the sum is divided by a per-Gaussian visibility count; this trainer keeps the reference's global step count, and
        nobody has tuned the value here.  Single-device steps; the reference strategy with densify on, or strategy="adc", where
        the absolute sums are averaged over the steps that saw the Gaussian, as in gsplat; composes with
        pose_opt, exposure_opt, bilateral_grid, filter_3d, contrib_prune, an anti-aliased renderer and referenceParamReload.
        Off (the default): no kernel, buffer or result differs.

        sparse_adam: the step updates only the Gaussians its view saw (include/gsplat.h gs_set_sparse_adam, DESIGN.md section 17;
        Taming 3DGS, Mallick et al. 2024: Inria's --optimizer_type sparse_adam, gsplat's visible_adam).  A Gaussian is visible in
        a step iff the step's forward gave it a radius > 0 (the renderer's N_visible).  A visible row gets the update it gets
        today -- on a zero gradient too, if no pixel blended it --; every element of an invisible row, parameter and both
        moments, keeps its bits, where dense Adam lets it drift on its momentum and lets its second moment decay.  The trainer
        turns the renderer's setting on around its own steps and puts it back.  fuse_adam=True: the fused backward + Adam skips
        the invisible rows (a wave of 64 invisible rows loads and stores nothing); fuse_adam=False: the step ends with
        gs_adam_step_visible on the forward's mask.  The densify statistic is what it is without the setting.  Composes with
        pose_opt, exposure_opt, bilateral_grid, absgrad, contrib_prune, an anti-aliased renderer, densify on or off and
        referenceParamReload; single-device steps with one view only, not with strategy='mcmc' (its noise and regularisers act
        on every Gaussian every step) and not with filter_3d.  Off (the default): no kernel, buffer or result differs.

        background: training on RGBA views over a background colour (background.BackgroundConfig, include/gsplat.h
        gs_set_background; Inria's --random_background, gsplat's backgrounds= / random_bkgd).  Every step
        takes trainStep's targetAlpha beside targetRGB (straight, un-premultiplied, as the loaders return them), picks the step's
        colour b -- background_for(seed, t) in mode "random", the configured colour in mode "fixed" --, sets it as the renderer's
        background, composites the target over it into a buffer the trainer owns (gs_composite_target) and runs the step on
        that target; a forward repeated for an overflow or a depth-cut miss runs under the same b.  Only a truly empty pixel
        then matches its target at every step, where a fixed black or white lets floaters of the background's colour go
        free.  The renderer's own background is put back behind the step; lastBackground holds b.  Mode "random" calls the
        loss without a target key (the target statistics cache cannot serve an image that changes every step); mode "fixed"
        keeps it.  The feature only sets a blend-level colour and swaps the target: it composes with pose_opt, exposure_opt,
        bilateral_grid, absgrad, sparse_adam, filter_3d, contrib_prune, strategy='mcmc', an anti-aliased renderer and fuse_adam
        on or off; single-device steps with one view only.  Off (the default): no kernel, buffer or result differs.

        depth: depth-supervised training (depth_loss.DepthConfig, include/gsplat.h gs_depth_loss; the
        reference's depth term, GaussianTrainer.swift:689-714 and :949, Inria's depth regularisation, gsplat's depth_loss).
        Every step takes trainStep's targetDepth (and depthMask, depthAlign), renders WITH the depth image and with the
        forward's depth sums checkpointed (depth_gradient = 1, put back behind the step), runs the colour loss as always and
        then gs_depth_loss on the render's depth and alpha in depth.mode -- "accumulated" (the reference's), "expected" (D / a)
        or "disparity" (a / D against an inverse depth) -- at depth.weight_at(iteration, iterationCount), and hands the two
        cotangents to the backward beside the colour's: renderBackwardAdam with fuse_adam, renderBackward without.  The depth
        loss sits where the colour loss does, so a forward repeated for an overflow or a depth-cut miss repeats it on the new
        images; the step's loss[3] is the depth term and loss[0] includes weight times it.  The depth term has its own mask,
        not lossMask.  It adds a loss and two cotangents the library's backwards already take: it composes with pose_opt,
        exposure_opt, bilateral_grid, absgrad, sparse_adam, filter_3d, contrib_prune, lossMask, background (whose g . b term the
        library adds to the alpha cotangent it is handed), strategy='mcmc', an anti-aliased renderer and fuse_adam on or off;
        single-device steps with one view only.  Off (the default): no kernel, launch, buffer or result differs, and the step
        still renders without a depth image.

        normal: normal regularisation from the rendered depth (normal_loss.NormalConfig, include/gsplat.h gs_normal_loss,
        DESIGN.md section 34; the normal terms of DN-Splatter, MonoSDF and VCR-GauS, the smoothness the surface methods beside
        mesh.extract_mesh train with).  From iteration normal.start on every step renders WITH the depth image under
        depth_gradient = 1 (put back behind the step, also when it raises), runs the colour loss as always, the depth term where
        depth= is set, and then gs_normal_loss on the render's depth and alpha: the L1 and cosine terms against trainStep's
        targetNormal (under normalMask) and the smoothness term between neighbouring pixels, weighted on the step's target
        colour by normal.edge_gamma.  A step without targetNormal runs the smoothness term alone.  The term's two cotangents go
        to the backward beside the colour's -- added to the depth term's where there is one, which then always writes an alpha
        cotangent, zeros in its accumulated mode --, a repeated forward repeats the term, loss[0] includes the weighted terms
        and lastNormalTerms holds (L_l1, L_cos, L_s).  Pinhole cameras only.  It composes with what depth= composes with;
        single-device steps with one view only.  Before normal.start, and with None (the default): no kernel, launch, buffer
        or result differs.

        distortion: the depth distortion loss (distortion.DistortionConfig, include/gsplat.h gs_render_distortion /
        gs_arm_distortion; 2DGS eq. 13, gsplat's distloss, which GOF, PGSR and RaDe-GS train with too).
        From iteration distortion.start on every step, once its forward is final -- behind the depth-cut miss check, so on the
        lists of the forward the backward runs on --, renders the distortion image D (renderDistortion), adds
        weight mean(v D) to loss[0] under the step's lossMask (distortionLoss; v = 1 without one) and arms the term
        (armDistortion): the step's usual backward then adds the term's gradient to the per-Gaussian rows between the blend
        backward and the projection backward (+ Adam), in front of the ADC statistic.  distortionTerm() is the last mean D.
        The forward need not render a depth image.  Pinhole cameras only.  It composes with every strategy, depth=, normal=,
        sparse_adam, sh_schedule, the per-view corrections, absgrad (whose absolute sums stay the colour and depth terms'),
        an anti-aliased renderer and fuse_adam on or off; single-device steps with one view only.  Before distortion.start,
        and with None (the default): no kernel, launch, buffer, setter call or result differs.

        strategy="adc", adc: adaptive density control, the densification of the original 3DGS (adc.ADCConfig, include/gsplat.h
        gs_set_adc_stats; Inria's densify_and_prune and reset_opacity, gsplat's DefaultStrategy) with the
        settings `adc` -- required, for its scene_extent (adc.scene_extent(cameras)).  The trainer owns three [N] accumulators
        and sets them as the renderer's ADC statistic around its steps up to densify_until: every such step's backward adds, for each Gaussian its view
        saw, hypot(W/2 gx, H/2 gy) of the 2-D mean gradient, one visit and the radius.  Behind steps densify_from <= t <=
        densify_until, t % densify_interval == 0 the event (_adcEvent): classify on the per-Gaussian average, splits sampled
        from the Gaussian itself, exact clones, the Adam moments of what survives kept, the accumulators zeroed; one host wait
        per event.  Behind steps t % opacity_reset_interval == 0 (t <= densify_until) the opacities are capped at reset_value,
        and from the first reset on the events also prune by screen and world size.  allowDensify = N < maxGaussians; an event
        that would still exceed maxGaussians only prunes.  The reference strategy is off (densify is ignored);
        lastDensifyStats holds the last event's counts, lastADCStats those and reset / size_prune.  With absgrad= the absolute
        sums are what is accumulated and absgrad.threshold replaces grad_threshold (gsplat's DefaultStrategy(absgrad=True)).
        Composes with pose_opt, exposure_opt, bilateral_grid, background, depth, lossMask, an anti-aliased renderer and
        fuse_adam on or off; single-device steps with one view only, not with filter_3d, contrib_prune, sparse_adam or
        referenceParamReload.

        sh_schedule: a progressive SH degree (sh_schedule.SHDegreeSchedule, include/gsplat.h gs_set_sh_degree, DESIGN.md section
        30; Inria's oneupSHdegree, gsplat's sh_degree_interval).  Before step t the trainer sets the renderer's active degree to
        sh_schedule.degree_at(t), capped at the renderer's maximum, when it differs; the degree only ever rises during a run,
        and lastSHDegree holds the running step's.  The model keeps its K: the bands above the active degree are not evaluated,
        their gradients are exact zeros, and the plain fused step (fuse_adam with none of pose_opt, strategy='mcmc', filter_3d
        and sparse_adam) leaves their bytes in the parameter and both moment arenas untouched and unread.  Every other form runs
        its full-row update on those zeros, which moves nothing: a band that has never been active has zero moments, and every
        event carries zeros as zeros.  evaluate, contribution scoring and the ADC and MCMC events render at the current degree;
        snapshots are written whole, the inactive bands as the model holds them.  Composes with every single-device feature and
        strategy through the form that feature already selects; single-device steps with one view only.  None (the default): no
        call, kernel or result differs."""
        # which switches are on, as _FEATURES' refusals name them
        on = dict(mcmc=strategy == "mcmc", adc=strategy == "adc", filter_3d=bool(filter_3d), sparse_adam=bool(sparse_adam),
                  contrib_prune=contrib_prune is not None, exposure_opt=bool(exposure_opt),
                  no_densify=not densify and strategy != "adc")
        where = (views_per_rank, process_group, dp_bootstrap, exchange_impl)

        def admit(feature, value=None, n_views=1):
            return None if value is None and _FEATURES[feature][0] else _admit(feature, value, on, where, n_views)

        self.lastSHDegree = None
        self._depthStep = None          # the running step's depth inputs (trainStep sets and clears it)
        self._normalStep = None         # the running step's normal term, from iteration normal.start on (the same)
        self._normalTerms = None        # (L_l1, L_cos, L_s) of the last step that ran the term, on the device
        self.lastBackground = None
        self._bgTarget = None
        self._bgSource = None
        self.sh_schedule, self.depth, self.normal = admit("sh_schedule", sh_schedule), admit("depth", depth), admit("normal", normal)
        self.distortion = admit("distortion", distortion)
        self._distortionStep = None     # the running step's distortion term, from iteration distortion.start on (as _normalStep)
        self._distortionBufs = None     # (D, totals, cot) on the device, allocated by the first step that runs the term
        self.background = admit("background", background)
        if not isinstance(sparse_adam, bool):
            raise ValueError("sparse_adam is True or False")
        self.sparse_adam = sparse_adam
        if sparse_adam:
            admit("sparse_adam")
        if strategy not in ("reference", "mcmc", "adc"):
            raise ValueError(f"unknown strategy {strategy!r} (\"reference\", \"mcmc\" or \"adc\")")
        self.strategy = strategy
        self.lastADCStats = None
        self.adcSizePrune = False       # size pruning: on once the first opacity reset has happened
        self._adcAcc = None             # [3, N]: gradSum, count, maxRadius
        if strategy == "adc" and adc is None:
            raise ValueError("strategy='adc' needs adc=ADCConfig(scene_extent=adc.scene_extent(cameras))")
        if strategy != "adc" and adc is not None:
            raise ValueError("adc settings need strategy='adc'")
        self.adc = admit("adc", adc)
        self.lastContribPruneStats = None
        self.contribPrune, self.absgrad = admit("contrib_prune", contrib_prune), admit("absgrad", absgrad)
        self.lastMCMCStats = None
        if strategy != "mcmc" and mcmc is not None:
            raise ValueError("mcmc settings need strategy='mcmc'")
        if strategy == "mcmc" and mcmc is None:
            from .mcmc import MCMCConfig
            mcmc = MCMCConfig()
        self.mcmc = admit("mcmc", mcmc)
        if self.mcmc is not None and self.mcmc.cap_max < model.N:
            raise ValueError(f"strategy='mcmc': cap_max = {self.mcmc.cap_max} is below the model's N = {model.N}")
        if strategy != "reference":
            densify = False             # (the strategy has its own events: the reference's are off)
        self.filter_3d = bool(filter_3d)
        if self.filter_3d:
            admit("filter_3d")
            if filter_cameras is None or len(filter_cameras) < 1:
                raise ValueError("filter_3d needs filter_cameras (the training cameras)")
            if isinstance(filter_3d_interval, bool) or int(filter_3d_interval) != filter_3d_interval or int(filter_3d_interval) < 1:
                raise ValueError("filter_3d_interval must be an integer >= 1")
        elif filter_cameras is not None:
            raise ValueError("filter_cameras need filter_3d=True")
        self.pose_opt = bool(pose_opt)
        if self.pose_opt:
            admit("pose_opt", n_views=n_views)
            if len(pose_lr) != 2:
                raise ValueError("pose_lr = (rotation rate, translation rate)")
        self.exposure_opt = bool(exposure_opt)
        if self.exposure_opt:
            admit("exposure_opt", n_views=n_views)
            try:
                elr = tuple(float(x) for x in exposure_lr)
            except (TypeError, ValueError):
                elr = ()
            if len(elr) != 2 or not all(math.isfinite(x) and x > 0.0 for x in elr):
                raise ValueError("exposure_lr = (initial rate, final rate), both positive and finite")
        self.bilateral_grid = bool(bilateral_grid)
        if self.bilateral_grid:
            admit("bilateral_grid", n_views=n_views)
            bgs = GaussianRenderer._grid_shape(bilateral_grid_shape, "bilateral_grid_shape")
            try:
                blr, btv = float(bilateral_grid_lr), float(bilateral_grid_tv)
            except (TypeError, ValueError):
                blr, btv = float("nan"), float("nan")
            if isinstance(bilateral_grid_lr, bool) or not (math.isfinite(blr) and blr > 0.0):
                raise ValueError("bilateral_grid_lr must be positive and finite")
            if isinstance(bilateral_grid_tv, bool) or not (math.isfinite(btv) and btv >= 0.0):
                raise ValueError("bilateral_grid_tv must be finite and >= 0")
        if dp_exchange not in ("sh_compressed", "allreduce"):
            raise ValueError(f"unknown dp_exchange {dp_exchange!r}")
        if exchange_impl not in ("torch", "native"):
            raise ValueError(f"unknown exchange_impl {exchange_impl!r}")
        if dp_bootstrap is not None and exchange_impl != "native":
            raise ValueError("dp_bootstrap = (id, rank, world) is the native exchange's bootstrap: pass exchange_impl='native' "
                             "(the torch exchange needs a process_group)")
        self.viewsPerRank = int(views_per_rank)
        if self.viewsPerRank < 1:
            raise ValueError("views_per_rank must be >= 1")
        if self.viewsPerRank > 1 and (dp_exchange != "sh_compressed" or exchange_impl != "torch"):
            raise ValueError("views_per_rank > 1 takes the sh_compressed exchange with the torch issuer (or no process group)")
        self.exchange_impl = exchange_impl
        self.model, self.gaussRender = model, gaussRender
        self.dp_exchange = dp_exchange
        self.iterationCount = iterationCount
        self.lambda_dssim = lambda_dssim
        self.pg = process_group
        self.world = 1
        self.rank = 0
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
            self.rank = dist.get_rank(process_group)
        if dp_bootstrap is not None:
            _, self.rank, self.world = dp_bootstrap
        r = gaussRender
        # without depth= this trainer's loss has no depth term (lambda_depth = 0, the reference's default:
        # GaussianTrainer.swift:280, 949), so no backward of ITS forwards ever brings a depth cotangent and they need not
        # checkpoint the depth sums: the knob is turned off around the trainer's own steps only (_trainStep) -- the renderer
        # is the caller's, and its other users keep whatever they had set.  With depth= it is turned on around them.
        self._loss = r._empty(4)
        self._cot = r._empty(r.H, r.W, 3)
        self._cotDepth = self._cotAlpha = None
        if self.depth is not None:
            self._cotDepth = r._empty(r.H, r.W)
            if self.depth.mode != "accumulated":      # (the accumulated depth has no cotangent into alpha)
                self._cotAlpha = r._empty(r.H, r.W)
        self._seg_end = self._segEnds()
        self.iteration = 0
        # densification (GaussianTrainer.swift:293-300, 304)
        self.gradientThreshold, self.minOpacity, self.maxScale = 0.0002, 0.005, 0.01
        if self.adc is not None:
            self.gradientThreshold, self.minOpacity = float(self.adc.grad_threshold), float(self.adc.min_opacity)
        if self.absgrad is not None:
            self.gradientThreshold = float(self.absgrad.threshold)
        self.densifyFromIter, self.densifyUntilIter, self.maxGaussians = 500, 15000, 1_000_000
        self.split_and_prune_per_iteration = 100
        self.densify = densify
        self.fuse_adam = fuse_adam                     # single-device steps: Adam inside the projection backward
        self.outputDirectory = None                    # set to a path to write iteration_<it>.ply snapshots
        self.save_snapshot_per_iteration = 100
        self.noise_seed = 20260313
        # Densify events WITHOUT a drain of the queue (round 5; single-device trainers -- a data-parallel one learns the count
        # behind its replica check anyway, and wants the packed layout): the count stays on the device for the kernels that
        # need it, the gather into a capacity-strided layout and the optimizer reset are queued BEFORE the host waits, and the
        # host waits for the event's plan alone (split_and_prune).  False: the reference's sequence to the letter -- read the
        # count, then size and queue everything behind it (one drain, ~0.3 ms of idle device per event).
        import os
        self.plannedDensify = os.environ.get("GSPLAT_PLANNED_DENSIFY", "1") != "0"      # (the switch: A/B runs of bench.py)
        # the split / clone noise: "torch" = torch.randn(total, 3) from a generator seeded by (noise_seed, iteration), what
        # rounds 1-4 drew; "library" = gs_densify_noise (row j a function of (seed, j) alone), what a planned event draws
        # inside its gather.  None: "library" where the event is planned, "torch" elsewhere.
        self.noiseSource = None
        self.xyzGradAccumulation = r._empty(model.N).zero_()
        self.denomGradAccumulation = 0
        self.lastDensifyStats = None
        self.forwardMisses = 0                         # forwards repeated without depth cuts (renderer.renderForward)
        # interval profiling (GaussianTrainer.swift:962-966, 1115-1127): every profilingLogInterval-th iteration runs
        # under an IntervalProfiler with the library's stage events on; lastProfileReport keeps its report
        self.enableIntervalProfiling = False
        self.profilingLogInterval = 100
        self.profilingTopKSections = 12
        self.lastProfileReport = None
        self.log = None                                # callable(str) for the reports, e.g. print
        self._committed = False
        # The reference re-reads `params` from the model every split_and_prune_per_iteration iterations whether or not
        # split_and_prune committed anything (GaussianTrainer.swift:1098-1110), and the model's tensors only change at a
        # commit (:900-905): outside the densify window, and at every cadence without a change, its training falls back to
        # the last committed state.  False (default): not mirrored -- training keeps what it has learnt.  True: the
        # reference's trajectory (a copy of the parameters is kept at every commit and restored at those points).
        self._referenceParamReload = False
        self._committed_params = None
        self.overflowRecoveries = 0                    # times the reserved pair capacity had to be regrown (see trainStep)
        self._checked_views = set()                    # views whose first forward has been checked for overflow
        # exchange_when_single: run the collectives even in a 1-rank group (exercises the RCCL path on one GPU)
        self._exchange = (process_group is not None or dp_bootstrap is not None) and (self.world > 1 or exchange_when_single)
        self._native = self._exchange and exchange_impl == "native"
        # the step takes the data-parallel FORM (split backward, gathered colour cotangents, SH rebuild, gate word in the
        # first payload) when it exchanges with other ranks or when this rank brings several views to it
        self._dp = self._exchange or self.viewsPerRank > 1
        # torch issuer: the step's all-gather as a synchronous op on the render stream where the backend is RCCL
        # (_gatherColourCotangents); GSPLAT_DP_INLINE_GATHER=0 keeps it on ProcessGroupNCCL's own stream (A/B)
        self.inlineGather = False
        if self._exchange and not self._native and process_group is not None:
            import torch.distributed as dist
            self.inlineGather = (dist.get_backend(process_group) == "nccl" and
                                 os.environ.get("GSPLAT_DP_INLINE_GATHER", "1") != "0")
        if self._native:
            self._dp_connect(dp_bootstrap)
        if self._dp and dp_exchange == "sh_compressed":
            if self.world * self.viewsPerRank > 16:
                raise ValueError("sh_compressed exchange supports at most 16 views per step (ranks x views_per_rank)")
        # data-parallel: a rank whose forward overflowed its reserved pairs must not be the only one to skip the Adam
        # step, or the replicas drift apart -- every optimizer kernel of a step tests the OR over the ranks of the
        # forwards' overflow words.  Round 5: the word rides in the step's first payload (behind the rank's colour
        # cotangents in the all-gather, whose words the SH rebuild ORs; behind the gradient arena in the all-reduce,
        # summed) -- rounds 3-4 gave it a 4-byte max all-reduce of its own, a third collective per step.
        #
        # And no rank may leave a step on its own: the host-side overflow error is turned off for the trainer's steps
        # (GS_TUNE_HOST_OVERFLOW_ERRORS), an optimizer kernel that finds the gate raised sets a `seen` word, and every
        # overflowCheckInterval-th step ALL ranks read it (one wait) -- it is built from the common gate, so they read the
        # same --, agree on the largest pair count any of them needed (a max all-reduce) and regrow their reserves together
        # (_collectiveOverflowCheck).  Steps in between were skipped by every replica's gate; nothing is applied from a
        # blank render.
        self._gate = None
        self.overflowCheckInterval = 16
        self._xt = None                                # exchange timing (exchangeTimingBegin / exchangeTimingRead)
        if self._dp and not self._native:               # (native: gs_dp_step keeps the gate, gs_dp_check_overflow the look)
            self._gate = torch.zeros(1, dtype=torch.int32, device=r.device)
            self._seen = torch.zeros(1, dtype=torch.int32, device=r.device)
            self._need = torch.zeros(1, dtype=torch.int64, device=r.device)
        self._alloc_exchange_buffers()
        if self.mcmc is not None:
            model.restride(max(self.mcmc.cap_max, model.capacity))
            self._seg_end = self._segEnds()
        # the enabled per-view corrections, in the order a step binds them and runs their Adam: pose, exposure, grid
        self._perView = {}
        eye = torch.eye(3, 4, dtype=torch.float32).reshape(12)        # [I | 0]: an exposure, a grid's node
        if self.pose_opt:
            self.nViews, self.poseLr = int(n_views), (float(pose_lr[0]), float(pose_lr[1]))
            # delta = (w, tau), zero to start; two segments at constant rates: rotation, translation
            self._perView["pose_opt"] = _PerViewTable("pose_opt", n_views, 6, r.device, (3, 6), lambda it, total: self.poseLr,
                                                      GaussianRenderer.setPoseCorrection)
            self._pose_delta = self._perView["pose_opt"].rows           # (the name the tests know the corrections by)
        if self.exposure_opt:
            self.nViews, self.exposureLr = int(n_views), elr
            self._perView["exposure_opt"] = _PerViewTable(
                "exposure_opt", n_views, 12, r.device, (12,), lambda it, total: (exposureLearningRate(it, total, self.exposureLr),),
                GaussianRenderer.setExposure, start=eye)
            self._expo_m, self._expo_v = self._perView["exposure_opt"].m, self._perView["exposure_opt"].v      # (likewise)
        if self.bilateral_grid:
            self.nViews, self.bilateralGridShape = int(n_views), bgs
            self.bilateralGridLr, self.bilateralGridTv = blr, btv
            # rows [grid_h, grid_w, grid_l, 12], the identity at every node to start
            nodes = bgs[0] * bgs[1] * bgs[2]
            self._perView["bilateral_grid"] = _PerViewTable(
                "bilateral_grid", n_views, nodes * 12, r.device, (nodes * 12,),
                lambda it, total: (bilateralGridLearningRate(it, total, self.bilateralGridLr),),
                lambda rr, G, g: rr.setBilateralGrid(G, g, self.bilateralGridShape, self.bilateralGridTv),
                start=eye.repeat(nodes), shared_grad=True)
            self._bg_m, self._bg_v = self._perView["bilateral_grid"].m, self._perView["bilateral_grid"].v      # (likewise)
        self._filter = None
        if self.filter_3d:
            self.filter3dInterval = int(filter_3d_interval)
            r.setFilterCameras(list(filter_cameras))
            self._updateFilter3D()
        if self._exchange:
            # the replicas must START identical too -- and the check's first call pays for the collective's set-up (a first
            # float64 max-reduce cost the torch exchange ~35 ms at the first densify event of a run) here, not there
            self.checkReplicas()
            if self._plans_events():      # ... likewise the plan check's side stream and its 16-word collective
                self.checkPlans(dict(zip(PLAN_WORDS, (model.N, 0, model.N, model.N, 0, 0, 0, model.N))))

    def _segEnds(self):
        """The arena's six segment ends as the Adam kernels take them."""
        return (C.c_longlong * 6)(*[int(x) for x in self.model.seg_end])

    @property
    def referenceParamReload(self):
        return self._referenceParamReload

    @referenceParamReload.setter
    def referenceParamReload(self, value):
        if value and self.mcmc is not None:
            raise ValueError("referenceParamReload mirrors the reference strategy's commits: not with strategy='mcmc'")
        if value and getattr(self, "adc", None) is not None:
            raise ValueError("referenceParamReload mirrors the reference strategy's commits: not with strategy='adc'")
        self._referenceParamReload = value

    def _updateFilter3D(self):
        """The filter widths of the model as it is now (gs_compute_filter3d), into the trainer's [capacity] buffer -- regrown
        with the model's capacity, so a steady-state step allocates nothing."""
        r, m = self.gaussRender, self.model
        need = max(int(m.capacity), int(m.N), 1)
        if self._filter is None or self._filter.numel() < need:
            self._filter = r._empty(need).zero_()
        r.computeFilter3D(m.getParams()["xyz"], out=self._filter)

    def filter3D(self) -> torch.Tensor:
        """The filter widths [N] of the current model (a view of the trainer's buffer)."""
        if not self.filter_3d:
            raise ValueError("filter3D: the trainer was built without filter_3d")
        return self._filter[:self.model.N]

    def _mcmcParams(self, iteration=None):
        """The gs_mcmc_params of step `iteration` (default: the coming one)."""
        return self.mcmc.params(self.iteration if iteration is None else iteration, self.noise_seed)

    def _mcmcEvent(self, it: int):
        """The MCMC strategy's event behind step `it` (include/gsplat.h gs_mcmc_relocate, gs_mcmc_grow): relocation, then
        growth into the rows behind N (the model is laid out at stride = capacity >= cap_max: nothing moves)."""
        r, m = self.gaussRender, self.model
        prm = self._mcmcParams(it)
        st = r.mcmcRelocate(m.getParams(), m.arena, m.m, m.v, prm)
        N0 = m.N
        N_new = r.mcmcGrow(m.getParams(), m.stride, m.arena, m.m, m.v, prm)
        if N_new != N0:
            m.setCount(N_new)
        self.lastMCMCStats = dict(dead=st["dead"], relocated=st["relocated"], added=N_new - N0, N=N_new)
        # rows moved or were added: the views' depth cuts no longer describe the scene.  No new layout: the rows were appended in
        # place at the stride the constructor laid out, and nothing of what a committed event resets belongs to this strategy
        self._afterCommit(N_new, grew=st["relocated"] > 0 or N_new != N0, layout=False, resetAccum=False)
        return self.lastMCMCStats

    # -- adaptive density control (adc.py, include/gsplat.h gs_set_adc_stats) --------------------------------
    def _adcAccumulators(self):
        """(gradSum, count, maxRadius), each [N]: rows of one zeroed tensor, allocated anew when N has changed."""
        if self._adcAcc is None or int(self._adcAcc.shape[1]) != self.model.N:
            self._adcAcc = self.gaussRender._empty(3, max(self.model.N, 1)).zero_()[:, :self.model.N]
        return self._adcAcc[0], self._adcAcc[1], self._adcAcc[2]

    def _adcEvent(self, it: int):
        """The ADC event behind step `it`: classify on the accumulators, densify.hip's scan and output map, the noise, the
        parameter gather and the moments' gather into staged buffers, commit, accumulators zeroed.  The unplanned sequence: one
        host wait (the output count).  Returns the action counts, or None for an empty model."""
        r, m, cfg = self.gaussRender, self.model, self.adc
        N = m.N
        if N <= 0:
            return None
        gradSum, count, maxRadius = self._adcAccumulators()
        p = m.getParams()

        def classify(allow):
            actions, counts = r.adcClassify(gradSum, count, maxRadius, p["scales"], p["opacity"].reshape(-1),
                                            gradThreshold=self.gradientThreshold, percentDense=cfg.percent_dense,
                                            minOpacity=self.minOpacity, maxScreenSize=cfg.max_screen_size,
                                            pruneWorld=cfg.prune_world, sceneExtent=cfg.scene_extent, allowDensify=allow,
                                            sizePrune=self.adcSizePrune)
            return (actions, counts) + r.densifyOffsets(actions, counts)

        allow = N < self.maxGaussians
        actions, counts, offsets, st = classify(allow)
        if allow and st["total"] > self.maxGaussians:
            allow = False                   # growing would pass maxGaussians: this event only prunes
            actions, counts, offsets, st = classify(allow)
        self.lastDensifyStats = st
        self.lastADCStats = dict(st, N=N, allow_densify=allow, reset=False, size_prune=self.adcSizePrune)
        total = st["total"]
        if total <= 0 or (st["split"] == 0 and st["clone"] == 0 and st["prune"] == 0):
            self._adcAcc.zero_()            # everything pruned, or nothing to do: the model stays, the statistic starts anew
            return st
        gather, mode = r.buildDensifyOutputMap(actions, offsets, total)
        noise = r.densifyNoise(self.noise_seed + int(it), total)
        r.adcGather(p, gather, mode, noise, revisedOpacity=cfg.revised_opacity, out=m.stagingViews(total))
        mOld, vOld = m.getMoments()
        mNew, vNew = m.stagingMoments()
        r.adcGatherMoments(mOld, gather, mode, actions, out=mNew)
        r.adcGatherMoments(vOld, gather, mode, actions, out=vNew)
        m.commitStaged(zero=False, moments=True)
        self._adcAcc = None                 # (the strategy's own statistic starts anew, not the reference's accumulator)
        self._adcAccumulators()
        self._afterCommit(total, grew=st["split"] > 0 or st["clone"] > 0, resetAccum=False)
        return st

    def _adcResetOpacity(self):
        """The opacity reset: opacity = min(opacity, logit(reset_value)), the opacity segment's moments zeroed; size pruning is
        on from here."""
        r, m = self.gaussRender, self.model
        if m.N > 0:
            mo, vo = m.getMoments()
            r.adcResetOpacity(m.getParams()["opacity"], mo["opacity"], vo["opacity"], self.adc.reset_value)
        self.adcSizePrune = True
        self.lastADCStats = dict(self.lastADCStats or {}, reset=True, size_prune=True)

    def _dp_connect(self, bootstrap):
        """gs_dp_init: rank 0 draws the RCCL id, every rank gets it (through process_group, whatever its backend), and the
        library creates its communicator on the renderer's device."""
        from . import _lib
        r = self.gaussRender
        if bootstrap is not None:
            uid = bytes(bootstrap[0])
        else:
            import torch.distributed as dist
            box = [None]
            if self.rank == 0:
                buf = C.create_string_buffer(_lib.GS_DP_UNIQUE_ID_BYTES)
                rc = r.lib.gs_dp_unique_id(buf)
                if rc != _lib.GS_OK:
                    raise GsplatError(rc, "gs_dp_unique_id failed (RCCL not loadable?)")
                box[0] = buf.raw
            dist.broadcast_object_list(box, src=dist.get_global_rank(self.pg, 0) if self.pg is not dist.group.WORLD else 0,
                                       group=self.pg)
            uid = box[0]
        r._check(r.lib.gs_dp_init(r.ctx, C.c_char_p(uid), int(self.rank), int(self.world)))

    def closeExchange(self):
        """Drops the library's communicator (native exchange); the renderer's close() does it too."""
        if self._exchange:
            self._resolveReplicaCheck()
        if self._native:
            self.gaussRender.lib.gs_dp_shutdown(self.gaussRender.ctx)
            self._native = self._exchange = False

    def _alloc_exchange_buffers(self):
        """The exchange's buffers for the model's current N, and -- torch exchange -- where the step's gate rides
        (gs_set_overflow_rider / gs_set_gathered_gate / gs_set_update_gate / gs_set_gate_seen; the native exchange does the
        same inside gs_dp_step).  Called again after every committed densify event: N and the arenas have moved."""
        if not self._dp:
            return
        r, m = self.gaussRender, self.model
        N = m.N
        V = self.viewsPerRank
        if self.dp_exchange == "sh_compressed":
            ccf = cc_block_floats(N)
            # this rank's V blocks one behind the other: what the all-gather hands over; without other ranks that buffer IS
            # the gathered one
            self._cc_local = r._empty(V * ccf)
            self._cc_all = r._empty(self.world * V, ccf) if self._exchange else self._cc_local.view(V, ccf)
            self._cc_local.view(V, ccf)[:, 3 * N:].zero_()
        if V > 1:
            # the geometry gradients of the rank's views, each laid out as the gradient arena's leading slice; their sum over
            # the views goes to that slice (zeroed once: a strided layout's rows between N and the stride are never written)
            self._geom_v = torch.zeros(V, m.geom_numel, dtype=torch.float32, device=r.device)
            self._geom_views = []
            for j in range(V):
                views = {}
                for k, off in zip(ARENA_ORDER[:4], m.seg_start[:4]):
                    views[k] = self._geom_v[j, int(off):int(off) + N * m._per[k]].view((N,) + m._row[k])
                self._geom_views.append(views)
            self._loss_v = r._empty(V, 4)
        if self._native:
            return
        if self.fuse_adam and self.dp_exchange == "sh_compressed":
            # the split form of round 6 (include/gsplat.h, gs_render_backward_dp_finish_geom): every view's xyz gradient without its
            # view-direction term, and that term summed over the step's views (the pad behind 3 N stays zero: Adam's last float4)
            x4 = (3 * N + 3) & ~3
            self._xyz_own = torch.zeros(V, x4, dtype=torch.float32, device=r.device)
            self._xyz_add = torch.zeros(x4, dtype=torch.float32, device=r.device)
        if self.dp_exchange == "sh_compressed":
            r._check(r.lib.gs_set_overflow_rider(r.ctx, C.c_void_p(self._cc_local.data_ptr() + 12 * N)))
            r._check(r.lib.gs_set_gathered_gate(r.ctx, cc_block_floats(N), int(self.world * V), _p(self._gate)))
            r._check(r.lib.gs_set_update_gate(r.ctx, _p(self._gate)))
        else:
            # the word behind the gradient arena (GaussModel keeps a spare one): stored by the backward, summed by the
            # all-reduce, tested -- as it lies -- by the Adam kernel (+0.0f is the all-zero word)
            word = C.c_void_p(m._gbuf.data_ptr() + 4 * m.numel)
            r._check(r.lib.gs_set_overflow_rider(r.ctx, word))
            r._check(r.lib.gs_set_gathered_gate(r.ctx, 0, 0, None))
            r._check(r.lib.gs_set_update_gate(r.ctx, word))
        r._check(r.lib.gs_set_gate_seen(r.ctx, _p(self._seen)))

    # -- densification bookkeeping (GaussianTrainer.swift:724-748) ------------------------------------------------
    def addGradientAccumulation(self, xyzGrad=None):
        """accum += |xyz_grad| of THIS rank's view (the reference accumulates per view, :1000); the per-rank
        accumulators are summed over ranks once, when split_and_prune needs them.  Inside trainStep the addition is
        fused into the projection backward (renderer.setGradNormAccum) and this only advances the denominator;
        called with a gradient it runs the stand-alone kernel.  A step the device gate skipped (reserved-capacity
        overflow) still counts in the denominator although its blank render added nothing: at most a few steps per
        regrown reserve, against a threshold that is a mean over ~100."""
        if xyzGrad is not None:
            if self.xyzGradAccumulation.shape[0] != int(xyzGrad.shape[0]):
                self.resetGradientAccumulation()
            self.gaussRender.accumGradNorm(xyzGrad, self.xyzGradAccumulation, out=self.xyzGradAccumulation)
        self.denomGradAccumulation += self.world

    def resetGradientAccumulation(self):
        self.xyzGradAccumulation = self.gaussRender._empty(self.model.N).zero_()
        self.denomGradAccumulation = 0

    def save_snapshot(self, iteration: int):
        """GaussianTrainer.swift:909-930: iteration_<it>.ply in the output directory, raw parameters."""
        import os
        from .ply import PlyWriter
        p = self.model.getParams()
        if self.filter_3d:       # the fused export: a viewer without the filter renders the filtered model
            p = self.gaussRender.bakeFilter3D(p, self._filter)
        PlyWriter(self.gaussRender).writeGaussianBinary(p["xyz"], p["features_dc"], p["features_rest"], p["opacity"],
                                                        p["scales"], p["rotation"],
                                                        to=os.path.join(os.fspath(self.outputDirectory),
                                                                        f"iteration_{iteration}.ply"))

    def prewarmDensify(self):
        """Dry run of the whole densify sequence on the current model (nothing is committed): loads the kernels,
        sizes the scan scratch and allocates the second parameter buffer, so the first real event costs what every
        later one does."""
        r, m = self.gaussRender, self.model
        if m.N <= 0:
            return
        p = m.getParams()
        acc = r._empty(m.N).zero_()
        actions, counts = r.classifyGaussians(acc, 1.0, p["scales"], p["opacity"].reshape(-1), self.gradientThreshold,
                                              self.maxScale, self.minOpacity, True)
        offsets, st = r.densifyOffsets(actions, counts)
        if st["total"] <= 0:
            return
        gather, mode = r.buildDensifyOutputMap(actions, offsets, st["total"])
        gen = torch.Generator(device=r.device)
        gen.manual_seed(self.noise_seed)
        noise = torch.randn(st["total"], 3, generator=gen, device=r.device, dtype=torch.float32)
        r.densifyGather(p, gather, mode, noise, out=m.stagingViews(st["total"]))
        m._staged = None
        if self._plans_events():      # ... and the planned form's kernels
            offsets = r.densifyPlan(actions, counts)
            gather, mode = r.buildDensifyOutputMapPlanned(actions, offsets, m.capacity)
            if self._dp:
                r.densifyGatherPlannedPacked(p, gather, mode, self.noise_seed, m.stagingBase(m.capacity), m.capacity, ARENA_ORDER)
            else:
                r.densifyGatherPlanned(p, gather, mode, self.noise_seed, m.stagingViews(m.capacity, stride=m.capacity), m.capacity)
            m._staged = None
            r.densifyPlanRead(wait=True)
            r.densifyNoise(self.noise_seed, 16)

    def _plans_events(self) -> bool:
        return bool(self.plannedDensify) and not self.referenceParamReload

    def _afterCommit(self, N_new: int, grew: bool, regrow: bool = True, layout: bool = True, resetAccum: bool = True,
                     keepForReload: bool = False):
        """What every event does once the model holds its N_new rows.  grew: rows were added (or moved).  New Gaussians
        lengthen the sweeps: a stale depth cut then costs a whole repeated forward, a fresh one 60 us of binning -- measured:
        every view missed once after such an event --, so the cuts go.  An event that only PRUNED (every event of a scene at
        the maxGaussians cap, GaussianTrainer.swift:300, 808) removes splats of opacity < 0.005: no sweep gets longer by more
        than the cuts' margin (2 x the sweep + 128 entries), and the cuts are depth keys, not indices, so the compaction of
        the arrays does not touch them.  They stay -- with 100 views and an event every 100 iterations every visit would
        otherwise be an uncut one (the 2 M garden scene: 1.85 instead of 0.47 ms of binning per step).  A cut that does miss
        is caught as ever (renderer.forwardMissed).
        regrow: a pair reserve made for fewer Gaussians grows in proportion, plus a tenth.  layout: the arena was laid out anew
        -- the event counts as committed, the segment ends and the exchange's buffers follow the new N.  resetAccum: the
        reference strategy's densify statistic starts anew.  keepForReload: under referenceParamReload the committed
        parameters are kept for the reload (the events that can run with it)."""
        r, m = self.gaussRender, self.model
        if layout:
            self._committed = True
        if keepForReload and self.referenceParamReload:
            self._committed_params = m.arena.clone()
        if grew:
            r.dropDepthCuts()
        if regrow and r.reserved is not None and N_new > r.reserved[0]:
            r.reserve(N_new, int(r.reserved[1] * (N_new / max(r.reserved[0], 1)) * 1.1))
        if layout:
            self._seg_end = self._segEnds()
            self._alloc_exchange_buffers()
        if resetAccum:
            self.resetGradientAccumulation()

    def _split_and_prune_planned(self, iteration: int, allowDensify: bool):
        """The event with the count left on the device (include/gsplat.h, gs_densify_plan; densify.hip).  Queued before the
        host waits for anything: classify, the scan and the plan, the output map and the gather for `capacity` slots into the
        other parameter buffer at CAPACITY strides (its pointers do not depend on the count), the optimizer reset.  Then the
        host waits for the PLAN -- the device still has the gather and the resets in front of it while the host lays the new
        model out and queues the next step.  The reference's early-outs (:819-847) are the plan's `applies` word: an event
        that changes nothing gathers the identity.  A new count beyond the capacity -- known before anything else is queued,
        the source buffer untouched -- repeats the map and the gather into a larger buffer."""
        r, m = self.gaussRender, self.model
        p = m.getParams()
        # Data-parallel form (round 6): the statistic's all-reduce is queued like any kernel (RCCL on its stream behind this
        # one's work, joined back: no host wait), the gather writes the PACKED layout -- tensor starts computed on the device
        # from the plan, since the step all-reduces the arena's leading geometry slice --, and the ranks compare their PLANS in
        # one fixed-size collective on a side stream as soon as the host has them (a diverged N is caught before the next
        # size-dependent collective without draining the queue); the arena checksum is queued behind the gather and its
        # verdict taken where the host waits anyway (_resolveReplicaCheck).
        packed = self._dp
        if self._exchange:
            self._resolveReplicaCheck()
            if self._native:
                r._check(r.lib.gs_dp_allreduce_sum(r.ctx, _p(self.xyzGradAccumulation), int(m.N)))
            else:
                import torch.distributed as dist
                dist.all_reduce(self.xyzGradAccumulation, op=dist.ReduceOp.SUM, group=self.pg)
        actions, counts = r.classifyGaussians(self.xyzGradAccumulation, float(self.denomGradAccumulation), p["scales"],
                                              p["opacity"].reshape(-1), self.gradientThreshold, self.maxScale,
                                              self.minOpacity, allowDensify)
        offsets = r.densifyPlan(actions, counts)
        seed = self.noise_seed + int(iteration)
        cap = m.capacity

        def gatherInto(cap):
            gather, mode = r.buildDensifyOutputMapPlanned(actions, offsets, cap)
            if packed:
                r.densifyGatherPlannedPacked(p, gather, mode, seed, m.stagingBase(cap), cap, ARENA_ORDER)
            else:
                r.densifyGatherPlanned(p, gather, mode, seed, m.stagingViews(cap, stride=cap), cap)

        gatherInto(cap)
        m.zeroOptimizerBuffers(grads=packed or not self.fuse_adam)      # the reference re-creates the optimizer state at every cadence
        plan = r.densifyPlanRead(wait=True)                   # the plan alone: the gather and the resets are still queued
        st = {k: plan[k] for k in ("total", "keep", "split", "clone", "prune")}
        self.lastDensifyStats = st
        if self._exchange:
            self.checkPlans(plan)                              # before anything is sized by this rank's own N_new
        N_new = plan["N_new"]
        if N_new > cap:
            cap = int(N_new * 1.5)
            gatherInto(cap)
            if not packed:
                m._staged = (cap, cap, cap)
        m.commitStaged(N_new=N_new, zero=False)
        self._afterCommit(N_new, grew=plan["applies"] and (st["split"] > 0 or st["clone"] > 0))
        if self._exchange:
            self.checkReplicas(deferred=True)      # queued behind the gather; the verdict where the host next waits
        return st

    def split_and_prune(self, iteration: int):
        """GaussianTrainer.swift:766-907.  Every rank runs it on identical inputs (parameters are replicated, the
        accumulators are all-reduced, the noise comes from a generator seeded by (noise_seed, iteration)), so the new
        model is identical on every rank with no further communication.  Returns the action counts or None."""
        if not (self.densifyFromIter <= iteration <= self.densifyUntilIter):
            return None
        r, m = self.gaussRender, self.model
        N = m.N
        if N <= 0:
            self.resetGradientAccumulation()
            return None
        allowDensify = N < self.maxGaussians
        if self.xyzGradAccumulation.shape[0] != N:
            self.resetGradientAccumulation()
        if self._plans_events() and (self.noiseSource or "library") == "library":
            return self._split_and_prune_planned(iteration, allowDensify)
        self._resolveReplicaCheck()
        if self._native:
            r._check(r.lib.gs_dp_allreduce_sum(r.ctx, _p(self.xyzGradAccumulation), int(N)))
        elif self._exchange:
            import torch.distributed as dist
            dist.all_reduce(self.xyzGradAccumulation, op=dist.ReduceOp.SUM, group=self.pg)
        p = m.getParams()
        actions, counts = r.classifyGaussians(self.xyzGradAccumulation, float(self.denomGradAccumulation), p["scales"],
                                              p["opacity"].reshape(-1), self.gradientThreshold, self.maxScale,
                                              self.minOpacity, allowDensify)
        offsets, st = r.densifyOffsets(actions, counts)
        self.lastDensifyStats = st
        total = st["total"]
        if total <= 0 or (st["split"] == 0 and st["clone"] == 0 and st["prune"] == 0):
            self.resetGradientAccumulation()          # all pruned (:828-832) or nothing to do (:819-826, :843-847)
            return st
        gather, mode = r.buildDensifyOutputMap(actions, offsets, total)
        noise = None
        if (st["split"] > 0 or st["clone"] > 0) and (self.noiseSource or "torch") == "library":
            noise = r.densifyNoise(self.noise_seed + int(iteration), total)
        elif st["split"] > 0 or st["clone"] > 0:
            gen = torch.Generator(device=r.device)
            gen.manual_seed(self.noise_seed + int(iteration))
            noise = torch.randn(total, 3, generator=gen, device=r.device, dtype=torch.float32)
        r.densifyGather(p, gather, mode, noise, out=m.stagingViews(total))
        m.commitStaged()
        self._afterCommit(total, grew=st["split"] > 0 or st["clone"] > 0, keepForReload=True)
        if self._exchange:
            self.checkReplicas()       # before the next size-dependent collective
        return st

    def _contribScores(self, cameras):
        """(max_w, sum_w) of the current model over `cameras`, rendered as a step renders them: the 3-D filter set, the learned
        pose of view i applied to cameras[i], no per-view correction bound.  A forward that overflowed the reserved pairs would
        score its view as blank: the reserve is regrown and the scoring repeated."""
        r, m = self.gaussRender, self.model
        cams = list(cameras)
        if self.pose_opt:
            cams = [self.refinedCamera(i, c) for i, c in enumerate(cams)]
        for t in self._perView.values():
            t.unbind(r)               # (a step binds its view's rows again; the refined cameras above carry the poses)
        def score():
            scores = r.contributionScores(m.getParams(), cams)
            r.sync()
            return scores

        with _Borrowed(r) as lent:
            if self.filter_3d:
                lent.set(filter_3d=self._filter)
            return self._retryOnOverflow(score)

    def _contribPruneEvent(self, cameras, threshold: float, score: str):
        """Scores the model over `cameras` and prunes what lies below the threshold through the densify event's machinery.
        Returns the stats; self._committed says whether the model changed."""
        r, m = self.gaussRender, self.model
        N = m.N
        st = dict(N=N, kept=N, pruned=0, threshold=float(threshold))
        self.lastContribPruneStats = st
        self._committed = False
        if N <= 0:
            return st
        maxW, sumW = self._contribScores(cameras)
        actions, counts = r.contribActions(maxW if score == "max" else sumW, float(threshold))
        p = m.getParams()
        if self._plans_events():
            offsets = r.densifyPlan(actions, counts)
            plan = r.densifyPlanRead(wait=True)
            if not plan["applies"] or plan["prune"] <= 0:      # nothing below the threshold, or everything: no change
                return st
            N_new, cap = plan["N_new"], m.capacity
            gather, mode = r.buildDensifyOutputMapPlanned(actions, offsets, cap)
            r.densifyGatherPlanned(p, gather, mode, self.noise_seed, m.stagingViews(cap, stride=cap), cap)
            m.commitStaged(N_new=N_new)
        else:
            offsets, ds = r.densifyOffsets(actions, counts)
            N_new = ds["total"]
            if N_new <= 0 or ds["prune"] <= 0:
                return st
            gather, mode = r.buildDensifyOutputMap(actions, offsets, N_new)
            r.densifyGather(p, gather, mode, None, out=m.stagingViews(N_new))
            m.commitStaged()
        # (nothing grew: the depth cuts stay, as after a densify event that only pruned, and no reserve is too small now)
        self._afterCommit(N_new, grew=False, regrow=False, keepForReload=True)
        st.update(kept=int(N_new), pruned=int(N - N_new))
        return st

    def pruneByContribution(self, cameras, threshold: float = 0.01, score: str = "max"):
        """The contrib_prune event on demand (e.g. compaction before save_snapshot): scores the model over `cameras`, prunes what
        lies below the threshold, resets the optimizer state as a committed densify event does.  Returns lastContribPruneStats.
        Single-device trainers with the reference strategy only."""
        from .contrib_prune import ContribPruneConfig
        if self.mcmc is not None:
            raise ValueError("pruneByContribution: the reference strategy only (not with strategy='mcmc')")
        if self._dp:
            raise ValueError("pruneByContribution: single-device steps only (no process group, dp_bootstrap, native exchange or "
                             "views_per_rank > 1)")
        cfg = ContribPruneConfig(threshold=threshold, at=(1,), cameras=list(cameras), score=score).validate()
        st = self._contribPruneEvent(cfg.cameras, cfg.threshold, cfg.score)
        if self._committed and self.filter_3d:
            self._updateFilter3D()
        return st

    def evaluate(self, cameras, targets, masks=None, targetAlphas=None, color_correct=None, viewKeys=None):
        """PSNR and SSIM of the current model over `cameras` against `targets` ([H, W, 3] each, the context's size): an
        evaluation.EvalResult.  Every view is rendered as a step renders it -- the 3-D filter set, the
        renderer's anti-aliasing mode as it is -- with renderChecked, and measured by gs_image_metrics: the sums of all views go
        to one [V, 4] device buffer that is read once at the end.

        viewKeys=None: held-out views.  No learnt pose and no per-view correction is applied, and the forwards are not keyed: a
        test view shares no depth cuts or hints with a training view.  viewKeys (one per camera): training views, rendered
        under their refined pose and measured under their trained exposure or grid (exposedRender / bilateralRender).
        masks: per view a uint8 (weight v / 255) or bool [H, W] image or None; pixels weigh in as in the masked training loss.
        color_correct: also cc_psnr / cc_ssim, the metrics after the least-squares affine colour transform of the (corrected)
        render onto the target; costs one read-back per view (the fit is on the host).  None: on exactly when the trainer
        trains an exposure or a bilateral grid.  targetAlphas: with a trainer built with background= (and only then) the views'
        alphas; render and target are composited over the config's fixed colour, black in the random mode.

        Trains nothing: the iteration counter, the arena, the densify accumulators and the loss's target caches are not
        touched, and the renderer's filter, background, pose binding and tuning knobs are put back whatever happens.
        Single-device trainers only."""
        from .evaluation import EvalResult, fit_affine_colour
        r, m = self.gaussRender, self.model
        if self._dp:
            raise ValueError("evaluate: single-device trainers only (no process group, dp_bootstrap, native exchange or views_per_rank > 1)")
        cams, tgts = list(cameras), list(targets)
        V = len(cams)
        per_view = dict(targets=tgts, masks=masks, targetAlphas=targetAlphas, viewKeys=viewKeys)
        for name, seq in per_view.items():
            if seq is not None and len(seq) != V:
                raise ValueError(f"evaluate: {name} has one entry per camera")
        if (targetAlphas is None) != (self.background is None):
            raise ValueError("evaluate: targetAlphas goes with a trainer built with background=BackgroundConfig(...)"
                             if self.background is None else
                             "evaluate: a trainer built with background= needs targetAlphas (the views' alphas, [H, W])")
        for t in tgts:
            if tuple(t.shape) != (r.H, r.W, 3):
                raise ValueError(f"evaluate: every target is [H, W, 3] = [{r.H}, {r.W}, 3], not {tuple(t.shape)}")
        cc = bool(self.exposure_opt or self.bilateral_grid) if color_correct is None else bool(color_correct)
        pose = self._perView.get("pose_opt")
        rows = None
        if viewKeys is not None and self._perView:
            rows = [next(iter(self._perView.values())).row(k) for k in viewKeys]
        bg = None
        if self.background is not None:
            bg = self.background.color_at(0) if self.background.mode == "fixed" else np.zeros(3, np.float32)
        sums = torch.zeros((V, 4), dtype=torch.float64, device=r.device)
        ccSums = torch.zeros((V, 4), dtype=torch.float64, device=r.device) if cc else None
        moments = torch.zeros(22, dtype=torch.float64, device=r.device) if cc else None

        def views():
            for i, cam in enumerate(cams):
                if pose is not None:
                    if rows is None:
                        pose.unbind(r)
                    else:
                        pose.bindRow(r, rows[i])      # (a forward reads the correction; only a backward writes its gradient)
                img = r.renderChecked(m.getParams(), cam, wantDepth=False).render
                if rows is not None and self.exposure_opt:
                    img = self.exposedRender(img, viewKeys[i])
                elif rows is not None and self.bilateral_grid:
                    img = self.bilateralRender(img, viewKeys[i])
                tgt = r._t(tgts[i])           # (uploaded once for the view's two or three calls, as is its mask)
                if bg is not None:
                    tgt = r.compositeTarget(tgt, targetAlphas[i], bg)
                mask = None if masks is None or masks[i] is None else r._metric_mask("evaluate", masks[i], r.H, r.W)
                r.imageMetrics(img, tgt, mask, out=sums[i])
                if cc:
                    M = fit_affine_colour(r.colourMoments(img, tgt, mask, out=moments).cpu().numpy())
                    # (the fit's p is the CLAMPED render: M is applied to that, and the metrics clamp M p again)
                    r.imageMetrics(r.applyExposure(img.clamp(0.0, 1.0), M), tgt, mask, out=ccSums[i])

        def measure():      # (a forward that overflowed the reserved pairs is blank: regrow, measure again)
            views()
            r.sync()

        # (the two knobs are the caller's whatever a forward's repeat does to them; the pose is bound view by view above)
        with _Borrowed(r, "depth_gradient", "host_overflow_errors", *(("pose",) if pose is not None else ())) as lent:
            if self.sh_schedule is not None:
                lent.set(sh_degree=self._scheduledSHDegree())      # (the degree the next step trains at)
            if self.filter_3d:
                lent.set(filter_3d=self._filter)
            if bg is not None:
                lent.set(background=bg)
            self._retryOnOverflow(measure)
            return EvalResult.from_sums(sums.cpu().numpy(), None if ccSums is None else ccSums.cpu().numpy())

    def checkReplicas(self, deferred: bool = False):
        """Every rank of a data-parallel job calls this at the same point (after every committed densify event): one
        fixed-size collective over (N, checksum, checksum of magnitudes) of the parameter arena; ReplicaMismatch on EVERY
        rank if the replicas differ -- a diverged N would otherwise hang the job in the next all-gather.
        deferred (round 6, the planned event): the checksum and its collective are QUEUED, the verdict is taken by
        _resolveReplicaCheck where the host next waits for the device anyway (the overflow look every overflowCheckInterval
        steps, the next event, closeExchange) -- the event does not drain the queue; what a hang would come from, a diverged
        count, checkPlans has caught at once."""
        r, m = self.gaussRender, self.model
        self._resolveReplicaCheck()
        if self._native:
            if deferred:
                r._check(r.lib.gs_dp_check_replicas_begin(r.ctx, int(m.N), _p(m.arena), int(m.numel)))
                self._replica_pending = True
                return
            self._replicaVerdict(r.lib.gs_dp_check_replicas(r.ctx, int(m.N), _p(m.arena), int(m.numel)))
        elif deferred:
            self._replica_pending = check_replicas_begin(m.N, m.arena, self.pg)
        else:
            check_replicas(m.N, m.arena, self.pg)

    def _replicaVerdict(self, rc):
        """The return code of one of the library's replica checks: ReplicaMismatch with its message, or any other error."""
        r = self.gaussRender
        if rc == GS_ERR_REPLICA_MISMATCH:
            raise ReplicaMismatch(r.lib.gs_last_error(r.ctx).decode())
        r._check(rc)

    def _resolveReplicaCheck(self):
        """The verdict of a deferred checkReplicas, if one is outstanding (every rank reaches this at the same points)."""
        pending, self._replica_pending = getattr(self, "_replica_pending", None), None
        if not pending:
            return
        if self._native:
            self._replicaVerdict(self.gaussRender.lib.gs_dp_check_replicas_end(self.gaussRender.ctx))
        else:
            check_replicas_end(pending, self.pg, self.rank)

    def checkPlans(self, plan: dict):
        """The ranks' densify plans compared (gs_dp_check_plan / check_plans): one fixed-size collective on a side stream, which
        does not wait for this stream's queue; ReplicaMismatch on EVERY rank unless all planned the same event."""
        words = [int(plan[k]) for k in PLAN_WORDS]
        if self._native:
            self._replicaVerdict(self.gaussRender.lib.gs_dp_check_plan(self.gaussRender.ctx, (C.c_longlong * 8)(*words), 8))
        else:
            if getattr(self, "_side", None) is None and self.gaussRender.device.type == "cuda":
                self._side = torch.cuda.Stream(device=self.gaussRender.device)
            check_plans(words, self.pg, self.gaussRender.device, getattr(self, "_side", None), self.rank)

    def _recover_overflow(self):
        """A forward needed more (Gaussian, tile) pairs than were reserved (include/gsplat.h, "Overflow"): the device
        gate has kept parameters and moments untouched for every step taken from such a forward, so nothing is
        corrupted -- regrow the reserve to 1.5x what was needed and carry on."""
        r = self.gaussRender
        r.lib.gs_sync(r.ctx)                              # waits; reports (and clears) the deferred error
        st = r.stats()
        need = int(st["M"]) if st["overflow"] else int(st["capM"])
        capN = max(int(st["capN"]), self.model.capacity)
        r.reserve(capN, max(int(need * 1.5) + 65536, int(st["capM"] * 1.5)))
        self.overflowRecoveries += 1

    def _retryOnOverflow(self, body, attempts: int = 4, recover: bool = True):
        """body(), repeated behind a regrown reserve while it raises GS_ERR_WORKSPACE_OVERFLOW: every regrow is by half at
        least, so a few rounds reach any need; the last attempt's error, and any other, is the caller's.  recover=False: no
        repeat at all (a data-parallel step never raises it -- host_overflow_errors is off, see __init__ -- and no rank may
        regrow on its own)."""
        for attempt in range(attempts):
            try:
                return body()
            except GsplatError as e:
                if e.code != GS_ERR_WORKSPACE_OVERFLOW or not recover or attempt == attempts - 1:
                    raise
                self._recover_overflow()

    def _overflow_reported(self) -> bool:
        """Has the device raised an overflow report that nobody has taken delivery of?  No wait: the report lives in host
        memory the device writes (gs_overflow_pending).  Behind a densify event -- whose count read has just waited for every
        forward queued before it -- that answer is complete, so the event needs no second wait to learn that nothing
        happened (round 3 called gs_sync there: a second drain of the queue per event)."""
        r = self.gaussRender
        rep = (C.c_uint32 * 2)()
        r._check(r.lib.gs_overflow_pending(r.ctx, rep))
        return rep[0] != 0

    def checkOverflow(self):
        """Waits for the device and regrows the pair reserve if any forward since the last check overflowed it.
        Returns True if it had to."""
        try:
            self.gaussRender.sync()
        except GsplatError as e:
            if e.code != GS_ERR_WORKSPACE_OVERFLOW:
                raise
            self._recover_overflow()
            return True
        return False

    def _collectiveOverflowCheck(self, force: bool = False):
        """Data-parallel: every rank calls this at the same iterations.  Reads the `seen` word the optimizer kernels set when
        the step's gate (the OR of every rank's overflow word, carried by the step's first collective) made them skip -- the
        same on every rank, one wait; if any step since the last check was gated, the ranks agree on the largest pair count
        needed and every one regrows its reserve to 1.5x that.  Returns True if it did."""
        r = self.gaussRender
        self._resolveReplicaCheck()           # (this look waits for the device anyway)
        if self._native:
            regrown, need = C.c_int(), C.c_longlong()
            r._check(r.lib.gs_dp_check_overflow(r.ctx, C.byref(regrown), C.byref(need)))
            if regrown.value:
                st = r.stats()
                r.reserved = (int(st["capN"]), int(st["capM"]))
                self.overflowRecoveries += 1
            return bool(regrown.value)
        import torch.distributed as dist
        if not force and not bool(self._seen.item()):
            return False
        # What to regrow to comes from the report of the forward that TRIPPED (the library keeps it until it is delivered),
        # not from the last forward's counters: the overflowing step need not be the last of the window, and with views
        # visited round-robin it never is for some views -- every rank would then compute "nothing needed", clear the word
        # and lose that view's steps again and again.
        # (the report is written by kernels on the CTX's stream -- the one the renderer captured when it was built, not
        # necessarily torch's current one: wait for THAT stream, or the report may not have landed, gs_sync below would then
        # deliver and clear it unseen, and the regrow would be sized from the last forward's counters after all)
        r._check(r.lib.gs_wait(r.ctx))
        rep = (C.c_uint32 * 2)()
        r._check(r.lib.gs_overflow_pending(r.ctx, rep))
        kind = int(rep[0])
        need = int(rep[1]) if kind == 1 else 0         # (the pair count belongs to a kind-1 report; a kind-2 one never wrote it)
        try:
            r.sync()                                   # takes delivery of (and clears) this rank's deferred report
        except GsplatError as e:
            if e.code != GS_ERR_WORKSPACE_OVERFLOW:
                raise
        st = r.stats()
        if kind == 0 and st["overflow"]:               # (the last forward itself, not yet reported)
            kind, need = 1, int(st["M"])
        if kind == 2:                                  # checkpoint arena: the pairs fitted; gs_ctx_reserve regrows the arena
            need = max(need, int(st["capM"]))
        elif kind == 0:
            need = 0
        self._need.fill_(need)
        dist.all_reduce(self._need, op=dist.ReduceOp.MAX, group=self.pg)
        need = int(self._need.item())
        self._seen.zero_()
        if need <= 0:
            return False
        capN = max(int(st["capN"]), self.model.capacity)
        # a rank whose own forwards fitted regrows too (need is the maximum over the ranks): replicas keep equal reserves
        r.reserve(capN, int(st["capM"]) if need <= int(st["capM"]) else max(int(need * 1.5) + 65536, int(st["capM"])))
        self.overflowRecoveries += 1
        return True

    # -- exchange timing (measurement only; bench.py's `exchange` block) ---------------------------------------------
    def _gatherColourCotangents(self, xt, inline=None):
        """The step's all-gather of the colour-cotangent blocks (+ gate words) through torch.distributed.  Where nothing is queued
        between it and the kernel that needs its result (the round-6 step: the SH kernel is next) and the backend is RCCL, it is
        issued as a SYNCHRONOUS op: ProcessGroupNCCL then launches it on the current -- the render -- stream itself, with no event
        hop to its own stream and back (1-rank group: 46 us of exposed wait -> the collective's own ~9; the library's issuer
        does the same through a split communicator, dp.hip).  Otherwise (gloo; a projection backward to hide it under) it is
        queued asynchronously and waited for where its result is needed.  Returns the Work to wait for, or None."""
        import torch.distributed as dist
        if inline is None:
            inline = self.inlineGather
        if inline:
            self._xt_mark(xt, "wg0")
            dist.all_gather_into_tensor(self._cc_all.view(-1), self._cc_local.view(-1), group=self.pg, async_op=False)
            self._xt_mark(xt, "wg1")
            return None
        gather = dist.all_gather_into_tensor(self._cc_all.view(-1), self._cc_local.view(-1), group=self.pg, async_op=True)
        if xt is not None:
            xt["work"].update(gather=gather)
        return gather

    def _awaitGather(self, gather, xt):
        if gather is not None:
            self._xt_mark(xt, "wg0")
            gather.wait()
            self._xt_mark(xt, "wg1")

    def exchangeTimingBegin(self):
        """From now on every data-parallel step is timed: how long each collective took and how long the render stream
        stood waiting for it (wire time NOT hidden under compute).  Native exchange: the library's own events around its
        RCCL calls (gs_dp_exchange_timing).  Torch exchange: events on the render stream around every Work.wait(), and the
        collectives' own durations from Work._get_duration() where the backend keeps them (ProcessGroupNCCL with
        TORCH_NCCL_ENABLE_TIMING=1; gloo does not)."""
        if not self._exchange:
            return
        r = self.gaussRender
        if self._native:
            r._check(r.lib.gs_dp_exchange_timing(r.ctx, 1))
        self._xt = []

    def _xt_step(self):
        if self._xt is None or self._native or len(self._xt) >= 512:
            return None
        st = dict(ev={}, work={})
        self._xt.append(st)
        return st

    @staticmethod
    def _xt_mark(st, name):
        if st is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            st["ev"][name] = e

    def exchangeTimingRead(self):
        """Per-step averages in ms since exchangeTimingBegin (waits for the device), or None if nothing was timed."""
        if self._xt is None:
            return None
        r, m = self.gaussRender, self.model
        if self._native:
            ms, steps, ver = (C.c_float * 8)(), C.c_int(), C.c_int()
            r._check(r.lib.gs_dp_exchange_read(r.ctx, ms, C.byref(steps), C.byref(ver)))
            r._check(r.lib.gs_dp_exchange_timing(r.ctx, 0))
            sums = dict(gate=ms[0], gather=ms[1], reduce=ms[2], exposed_gather=ms[3], exposed_reduce=ms[4])
            counts = dict(gate=steps.value, gather=steps.value, reduce=steps.value)
            n, version = steps.value, ver.value
            source = ("HIP events on the library's side stream around each RCCL call, and on the ctx stream around its "
                      "hipStreamWaitEvent on them (gs_dp_exchange_read)")
        else:
            torch.cuda.synchronize(r.device)
            n = len(self._xt)
            sums = dict(gate=0.0, gather=0.0, reduce=0.0, exposed_gather=0.0, exposed_reduce=0.0)
            counts = dict(gate=0, gather=0, reduce=0)
            for st in self._xt:
                ev = st["ev"]
                for a, b, k in (("wg0", "wg1", "exposed_gather"), ("wr0", "wr1", "exposed_reduce")):
                    if a in ev and b in ev:
                        sums[k] += ev[a].elapsed_time(ev[b])
                for k, w in st["work"].items():
                    try:
                        sums[k] += float(w._get_duration())
                        counts[k] += 1
                    except Exception:
                        pass
            try:
                import torch.cuda.nccl as _nccl
                v = _nccl.version()
                version = v[0] * 10000 + v[1] * 100 + v[2] if isinstance(v, tuple) else int(v)
            except Exception:
                version = None
            source = ("torch.cuda events on the render stream around every Work.wait(); collective durations from "
                      "Work._get_duration() (null where the backend keeps none)")
        self._xt = None
        return exchange_summary(self.exchange_impl, self.dp_exchange, self.world, m.N, int(m.geom_numel), int(m.numel), n, sums,
                                counts, version, source, self.viewsPerRank)

    def trainStep(self, camera, targetRGB, stepCameras=None, viewKey=None, targetAlpha=None, lossMask=None, targetDepth=None,
                  depthMask=None, depthAlign=(1.0, 0.0), targetNormal=None, normalMask=None):
        """One iteration: forward, loss, backward, (gradient exchange), Adam.  Asynchronous; returns the device
        loss[4].  stepCameras: the cameras of ALL ranks for this step in rank order (every rank derives them from the
        shared view permutation, see view_for), or just their centres [R,3]; required by the sh_compressed exchange.
        viewKey: identifies the training view (renderer.renderForward): enables the forward's deepest-first order.
        camera: a Camera(model="fisheye") is rendered and differentiated through the equidistant model, view
        by view beside pinhole ones; single-device steps with one view only, not with pose_opt or filter_3d.

        Reserved-capacity overflow: the step's calls raise GS_ERR_WORKSPACE_OVERFLOW as soon as the host sees the
        device's flag (at the latest at the checks below: the first visit of every view, every densify cadence); the
        reserve is regrown and the step repeated once.  Steps queued in between were skipped on the device (no
        optimizer update from a blank render), never applied.

        targetAlpha: the view's alpha, [H, W], with a trainer built with background= (and only then): targetRGB is then the
        view's straight colour, and the step's target their composite over the step's background.

        lossMask: regions of this view to ignore (include/gsplat.h gs_set_loss_mask; gsplat's masks=,
        Inria's alpha_mask): a uint8 (weight v / 255: 255 keeps a pixel, 0 ignores it, between is a soft edge) or bool (0 / 255)
        image [H, W], tensor or array.  It is bound to the renderer for the step's forwards and losses -- a forward repeated for
        an overflow or a depth-cut miss included -- and the renderer's previous mask is put back behind the step.  The step's
        colour loss is that of the weighted render and target, still divided by all 3 H W elements (no re-normalisation by the
        mask's coverage: a kept pixel's gradient has the scale it has without a mask), and its cotangent is exactly zero where
        the mask is: an ignored region moves no Gaussian, trains no exposure or grid and adds nothing to a densify statistic.
        A uint8 device tensor that stays where it is keeps the view's target statistics cached; a host array is uploaded anew
        every step and refills them.  Needs no constructor argument; composes with pose_opt, exposure_opt, bilateral_grid,
        absgrad, sparse_adam, filter_3d, contrib_prune, background, strategy='mcmc', an anti-aliased renderer and fuse_adam on
        or off; single-device steps with one view only.  None (the default): no kernel, buffer or result differs.

        targetDepth: the view's depth map, [H, W], with a trainer built with depth= (and only then): a metric depth in the
        accumulated and expected modes, an inverse depth in the disparity mode.  depthMask: uint8 or bool [H, W], non-zero =
        the pixel takes part in the depth term; None means targetDepth > 0 (sensor holes are 0).  depthAlign = (scale, offset):
        the term compares with scale * targetDepth + offset (Inria's depth_params.json pair; TrainData.depthAlign).

        targetNormal: the view's normal prior, [H, W, 3] in camera space (OpenCV axes, facing the camera; TrainData.normalArray),
        with a trainer built with normal= (and only then); a pixel of squared norm < 0.25 is a hole.  None: the step runs the
        smoothness term alone.  normalMask: uint8 or bool [H, W], non-zero = the pixel takes part in the prior terms; None = all.
        The smoothness pairs are weighted on the step's target colour (normal.edge_gamma)."""
        if getattr(camera, "model", "pinhole") == "fisheye":
            # (include/gsplat.h gs_set_camera_model: the fisheye model has no pose, filter or data-parallel kernels)
            for on, name in ((self.pose_opt, "pose_opt"), (self.filter_3d, "filter_3d")):
                if on:
                    raise ValueError(f"trainStep: a fisheye camera does not go with {name} (pinhole cameras only)")
            if self.pg is not None or self.exchange_impl == "native":
                raise ValueError("trainStep: a fisheye camera takes single-device steps only (no process group, dp_bootstrap or "
                                 "native exchange)")
            if self.viewsPerRank != 1:
                raise ValueError("trainStep: a fisheye camera takes one view per step only (views_per_rank > 1 is not supported)")
        if lossMask is not None:
            if self.viewsPerRank != 1:
                raise ValueError("trainStep: lossMask takes one view per step only (views_per_rank > 1 is not supported)")
            if self.pg is not None or self.exchange_impl == "native":
                raise ValueError("trainStep: lossMask takes single-device steps only (no process group, dp_bootstrap or native exchange)")
        if (targetAlpha is None) != (self.background is None):
            raise ValueError("trainStep: targetAlpha goes with a trainer built with background=BackgroundConfig(...)"
                             if self.background is None else
                             "trainStep: a trainer built with background= needs targetAlpha (the view's alpha, [H, W])")
        depth = self.depth
        if (targetDepth is None) != (depth is None):
            raise ValueError("trainStep: targetDepth goes with a trainer built with depth=DepthConfig(...)"
                             if depth is None else
                             "trainStep: a trainer built with depth= needs targetDepth (the view's depth map, [H, W])")
        if depth is None and depthMask is not None:
            raise ValueError("trainStep: depthMask goes with a trainer built with depth=DepthConfig(...)")
        normal = self.normal
        if normal is None and (targetNormal is not None or normalMask is not None):
            raise ValueError("trainStep: targetNormal and normalMask go with a trainer built with normal=NormalConfig(...)")
        if normal is not None and getattr(camera, "model", "pinhole") != "pinhole":
            raise ValueError("trainStep: normal= takes pinhole cameras only (the normals of a depth image are taken along "
                             "pinhole rays; a fisheye camera is not served)")
        normalOn = normal is not None and self.iteration >= normal.start
        distortion = self.distortion
        if distortion is not None and getattr(camera, "model", "pinhole") != "pinhole":
            raise ValueError("trainStep: distortion= takes pinhole cameras only (the depth of a fisheye record is a ray length, "
                             "which the maps are not defined on; a fisheye camera is not served)")
        profiled = self.enableIntervalProfiling and (self.iteration % self.profilingLogInterval == 0
                                                     or self.iteration == self.iterationCount - 1)
        step = self._profiledStep if profiled else (self._trainStepMulti if self.viewsPerRank > 1 else self._trainStep)
        r = self.gaussRender
        # what this step changes of the caller's renderer, put back whatever happens.  Held from the start: the two knobs, the
        # background (the target is composited before anything is set) and, with strategy='adc', the statistic _beginIteration sets
        keep = ["depth_gradient", "host_overflow_errors"]
        if self.adc is not None:
            keep.append("adc_stats")
        if self.background is not None:
            # the step's colour: the renderer's background for every forward of the step, and the target over it
            b = self.background.color_at(self.iteration)
            keep.append("background")
            targetRGB = self._compositeTarget(targetRGB, targetAlpha, b)
        tables = list(self._perView.values())
        row = tables[0].row(viewKey) if tables else None       # (one n_views for all of them)
        with _Borrowed(r, *keep, unbind=tables) as lent:
            try:
                if depth is not None:
                    self._depthStep = self._depthInputs(targetDepth, depthMask, depthAlign)
                lent.set(depth_gradient=0 if depth is None and not normalOn else 1)
                if normalOn:
                    self._normalStep = self._normalInputs(camera, targetRGB, targetNormal, normalMask)
                if distortion is not None and self.iteration >= distortion.start:
                    self._distortionStep = self._distortionInputs()
                if self.mcmc is not None:      # the strategy's step in the fused backward + Adam (the unfused step calls the ops)
                    lent.set(mcmc=self._mcmcParams())
                if self.filter_3d:
                    lent.set(filter_3d=self._filter)
                if self.sparse_adam and not r.sparseAdam:       # (a caller's renderer that has it on keeps it on)
                    lent.set(sparse_adam=True)
                if self.background is not None:
                    lent.set(background=b)
                    self.lastBackground = b
                for t in tables:
                    t.bindRow(r, row)
                if lossMask is not None:
                    lent.set(loss_mask=lossMask)
                if self._exchange:
                    lent.set(host_overflow_errors=0)
                    if self.iteration % self.overflowCheckInterval == 0 and self.iteration > 0:
                        self._collectiveOverflowCheck()
                return self._retryOnOverflow(lambda: step(camera, targetRGB, stepCameras, viewKey), recover=not self._exchange)
            finally:
                self._depthStep = self._normalStep = self._distortionStep = None

    def _distortionInputs(self):
        """The step's gs_distortion_params and weight.  The first step that runs the term allocates its three images: D, the
        pixels' totals and the cotangent."""
        r, cfg = self.gaussRender, self.distortion
        if self._distortionBufs is None:
            self._distortionBufs = (r._empty(r.H, r.W), r._empty(r.H, r.W, 3), r._empty(r.H, r.W))
        return dict(params=cfg.params(), weight=float(cfg.weight))

    def _distortionLoss(self, lossOut):
        """The distortion term of the step's FINAL forward (behind the depth-cut miss check: its lists are the ones the backward
        sweeps): D and the totals, weight mean(v D) into lossOut[0] under the step's loss mask, and the term armed for the
        step's backward."""
        r, d = self.gaussRender, self._distortionStep
        D, totals, cot = self._distortionBufs

        def body():
            r.renderDistortion(d["params"], D, totals)
            r.distortionLoss(D, d["weight"], r.lossMask, lossOut, cot)
            r.armDistortion(cot, totals, d["params"])
        r._measure("train.loss.distortion", body)

    def distortionTerm(self):
        """The mean of the distortion image D over all pixels (no mask, no weight) of the last step that ran the term, a 0-dim
        device tensor; None before the first."""
        return None if self._distortionBufs is None else self._distortionBufs[0].mean()

    def _depthInputs(self, targetDepth, depthMask, depthAlign):
        """The step's depth target and mask on the device and its gs_depth_loss_params."""
        r = self.gaussRender
        try:
            scale, offset = (float(x) for x in depthAlign)
        except (TypeError, ValueError):
            scale = offset = float("nan")
        if not (math.isfinite(scale) and math.isfinite(offset)):
            raise ValueError("trainStep: depthAlign = (scale, offset), both finite")
        td = r._t(targetDepth)
        if td.numel() != r.H * r.W or td.dim() not in (2, 3):
            raise ValueError(f"trainStep: targetDepth is [H, W] = [{r.H}, {r.W}]")
        if depthMask is None:
            dm = (td > 0).to(torch.uint8)          # sensor holes are 0; taken anew every step, from the map the step was given
        else:
            dm = depthMask if torch.is_tensor(depthMask) else torch.as_tensor(np.ascontiguousarray(depthMask))
            if dm.dtype not in (torch.uint8, torch.bool) or dm.numel() != r.H * r.W:
                raise ValueError(f"trainStep: depthMask is a uint8 or bool [H, W] = [{r.H}, {r.W}] image, or None")
            dm = dm.to(device=r.device, dtype=torch.uint8).contiguous()
        params = r.depthLossParams(self.depth.mode, self.depth.weight_at(self.iteration, self.iterationCount), self.depth.alpha_min,
                                   scale, offset)
        return dict(target=td, mask=dm, params=params)

    def _depthLoss(self, res, lossOut):
        """gs_depth_loss behind the colour loss that wrote lossOut: lossOut[3], lossOut[0] and the step's two cotangents."""
        r, d = self.gaussRender, self._depthStep
        r._measure("train.loss.depth", lambda: r.depthLoss(
            res.depth, None if self._cotAlpha is None else res.alpha, d["target"], d["mask"], d["params"],
            out=dict(loss=lossOut, cotDepth=self._cotDepth, cotAlpha=self._cotAlpha)))

    def _normalInputs(self, camera, targetRGB, targetNormal, normalMask):
        """The step's normal prior, mask and edge image on the device and its gs_normal_loss_params.  The first step that runs
        the term allocates what it needs: the two cotangent images (where depth= has not) and the three terms."""
        r, cfg = self.gaussRender, self.normal
        tn = nm = None
        if targetNormal is not None:
            tn = r._t(targetNormal)
            if tn.numel() != 3 * r.H * r.W:
                raise ValueError(f"trainStep: targetNormal is [H, W, 3] = [{r.H}, {r.W}, 3]")
        if normalMask is not None:
            nm = normalMask if torch.is_tensor(normalMask) else torch.as_tensor(np.ascontiguousarray(normalMask))
            if nm.dtype not in (torch.uint8, torch.bool) or nm.numel() != r.H * r.W:
                raise ValueError(f"trainStep: normalMask is a uint8 or bool [H, W] = [{r.H}, {r.W}] image, or None")
            nm = nm.to(device=r.device, dtype=torch.uint8).contiguous()
        l1, cos, smooth = cfg.weights_at(self.iteration, self.iterationCount)
        params = r.normalLossParams(camera, l1, cos, smooth, cfg.alpha_min, cfg.max_jump, cfg.edge_gamma,
                                    accumulate=self._depthStep is not None)
        edge = r._t(targetRGB) if cfg.edge_gamma > 0.0 and smooth > 0.0 else None
        if self._cotDepth is None:
            self._cotDepth = r._empty(r.H, r.W)
        if self._cotAlpha is None:      # (with depth= in the accumulated mode too: its term then writes the zeros this one adds to)
            self._cotAlpha = r._empty(r.H, r.W)
        if self._normalTerms is None:
            self._normalTerms = r._empty(3)
        return dict(camera=camera, target=tn, mask=nm, edge=edge, params=params)

    def _normalLoss(self, res, lossOut):
        """gs_normal_loss behind the colour loss that wrote lossOut, and behind the depth term where there is one (its cotangents
        are then added to): lossOut[0], self._normalTerms and the step's two cotangents."""
        r, d = self.gaussRender, self._normalStep
        r._measure("train.loss.normal", lambda: r.normalLoss(
            res.depth, res.alpha, d["camera"], d["target"], d["mask"], d["edge"], d["params"],
            out=dict(loss=lossOut, terms=self._normalTerms, cotDepth=self._cotDepth, cotAlpha=self._cotAlpha)))

    @property
    def lastNormalTerms(self):
        """(L_l1, L_cos, L_s) of the last step that ran the normal term, a device tensor; None before the first."""
        return self._normalTerms

    def _compositeTarget(self, targetRGB, targetAlpha, b):
        """The step's target: targetRGB over b by targetAlpha, in the trainer's own buffer (allocated once)."""
        r = self.gaussRender
        rgb, alpha = r._t(targetRGB), r._t(targetAlpha)
        if rgb.dim() != 3 or rgb.shape[-1] != 3 or tuple(alpha.shape) != tuple(rgb.shape[:2]):
            raise ValueError("trainStep: targetRGB is [H, W, 3] and targetAlpha [H, W]")
        if self._bgTarget is None or self._bgTarget.shape != rgb.shape:
            self._bgTarget = torch.empty_like(rgb)
        # what the composite was made of: the buffer is one for all views and is written behind torch's back, so its own identity
        # (which the renderer's target statistics cache checks) says nothing about the image it holds
        self._bgSource = (rgb.data_ptr(), rgb._version, alpha.data_ptr(), alpha._version, tuple(rgb.shape)) + tuple(float(x) for x in b)
        return r.compositeTarget(rgb, alpha, b, out=self._bgTarget)

    def _lossTargetKey(self, viewKey):
        """The key the loss caches the target's statistics under: none where the target changes every step (mode "random"); in
        mode "fixed" the view key together with the identity of the RGBA tensors and the colour the composite was made of, so that
        another image behind the key, an in-place write to it or another colour is a cache miss, as a rewritten target is without
        the feature (device tensors that stay where they are hit; a host array is uploaded anew every step and never does)."""
        if self.background is None or viewKey is None:
            return viewKey
        if self.background.mode == "random":
            return None
        return ("background", viewKey) + self._bgSource

    def _table(self, who: str, feature: str) -> _PerViewTable:
        if feature not in self._perView:
            raise ValueError(f"{who}: the trainer was built without {feature}")
        return self._perView[feature]

    def exposures(self) -> np.ndarray:
        """The views' exposures M = [A | b], host float32 [n_views, 3, 4] (waits for the device)."""
        t = self._table("exposures", "exposure_opt")
        return t.rows.cpu().numpy().reshape(t.nViews, 3, 4)

    def exposedRender(self, render, viewKey):
        """A render of view `viewKey` under the view's learned exposure (A render + b; gs_apply_exposure), a new tensor."""
        t = self._table("exposedRender", "exposure_opt")
        return self.gaussRender.applyExposure(render, t.rows[t.row(viewKey)])

    def bilateralGrids(self) -> np.ndarray:
        """The views' grids, host float32 [n_views, grid_h, grid_w, grid_l, 12] (each node an M = [A | b]; waits for the device)."""
        t = self._table("bilateralGrids", "bilateral_grid")
        gw, gh, gl = self.bilateralGridShape
        return t.rows.cpu().numpy().reshape(t.nViews, gh, gw, gl, 12)

    def bilateralRender(self, render, viewKey):
        """A render of view `viewKey` under the view's learned grid (gs_apply_bilateral_grid), a new tensor."""
        t = self._table("bilateralRender", "bilateral_grid")
        return self.gaussRender.applyBilateralGrid(render, t.rows[t.row(viewKey)], self.bilateralGridShape)

    def poseCorrections(self) -> np.ndarray:
        """The views' pose corrections delta = (w, tau), host float32 [n_views, 6] (waits for the device)."""
        return self._table("poseCorrections", "pose_opt").rows.cpu().numpy()

    def refinedCamera(self, viewKey, camera):
        """The view's camera with its learned correction applied (camera.apply_pose_correction, float64)."""
        from .camera import apply_pose_correction
        t = self._table("poseCorrections", "pose_opt")
        return apply_pose_correction(camera, self.poseCorrections()[t.row(viewKey)])

    def _profiledStep(self, camera, targetRGB, stepCameras, viewKey):
        """One iteration under the reference's IntervalProfiler: host sections by wall clock, device stages by the
        library's HIP events (this iteration waits for the device at its end; the others never do)."""
        import time
        from .profiler import IntervalProfiler
        r = self.gaussRender
        prof = IntervalProfiler(True)
        r.profiler = prof
        it = self.iteration
        t0 = time.perf_counter_ns()
        r.profile(True)
        try:
            body = self._trainStepMulti if self.viewsPerRank > 1 else self._trainStep
            out = prof.measure("train.valueAndGrad.execute", lambda: body(camera, targetRGB, stepCameras, viewKey))
            prof.setDeviceStages(r.profileRead())
        finally:
            r.profile(False)
            r.profiler = None
        self.lastProfileReport = prof.makeReport(it, time.perf_counter_ns() - t0, self.profilingTopKSections, 0.01)
        self.lastProfiler = prof
        if self.log:
            self.log(self.lastProfileReport)
        return out

    def _nativeStep(self, stepCameras):
        """Backward + exchange + Adam of this step through gs_dp_step (the library issues the RCCL calls)."""
        from . import _lib
        r, m = self.gaussRender, self.model
        a = _lib.gs_dp_step_args()
        a.cot_color, a.cot_depth, a.cot_alpha = self._cot.data_ptr(), None, None
        a.params_base, a.grads_base, a.m_base, a.v_base = (t.data_ptr() for t in (m.arena, m.grad, m.m, m.v))
        a.n_arena, a.geom_numel, a.nseg = int(m.numel), int(m.geom_numel), 6
        for i, (e, lr) in enumerate(zip(m.seg_end, arenaLearningRates(self.iteration, self.iterationCount))):
            a.seg_end[i], a.seg_lr[i] = int(e), float(lr)
        a.beta1, a.beta2, a.eps = ADAM_BETA1, ADAM_BETA2, ADAM_EPS
        mode = _lib.GS_DP_ALLREDUCE
        if self.dp_exchange == "sh_compressed":
            if stepCameras is None or len(stepCameras) != self.world:
                raise ValueError("sh_compressed exchange needs stepCameras (one camera per rank, rank order)")
            centres = np.ascontiguousarray(np.stack([np.asarray(getattr(c, "cameraCenter", c), np.float32).reshape(3)
                                                     for c in stepCameras]), np.float32)
            a.cam_centers = centres.ctypes.data
            a.color_cot_local, a.color_cot_all = self._cc_local.data_ptr(), self._cc_all.data_ptr()
            mode = _lib.GS_DP_SH_COMPRESSED
        r._cuts_renewed()
        r._check(r.lib.gs_dp_step(r.ctx, mode, C.byref(a)))

    def _scheduledSHDegree(self):
        """The active degree of the step about to run: the schedule's, never below a degree this run has already trained at."""
        d = self.sh_schedule.degree_at(self.iteration, self.gaussRender.maxSHDegree)
        return d if self.lastSHDegree is None else max(d, self.lastSHDegree)

    def _beginIteration(self):
        r, m = self.gaussRender, self.model
        if self.sh_schedule is not None:
            self.lastSHDegree = self._scheduledSHDegree()
            if r.shDegree != self.lastSHDegree:
                r.setSHDegree(self.lastSHDegree)
        if self.referenceParamReload and self._committed_params is None:
            self._committed_params = m.arena.clone()      # what the reference's model holds: the tensors before any step
        if self.densify:
            if self.xyzGradAccumulation.shape[0] != m.N:
                self.resetGradientAccumulation()
            if getattr(r, "_grad_norm_accum", None) is not self.xyzGradAccumulation:
                r.setGradNormAccum(self.xyzGradAccumulation)      # the backward below adds this view's |grad xyz|
        elif getattr(r, "_grad_norm_accum", None) is not None:
            r.setGradNormAccum(None)
        if self.absgrad is not None and not getattr(r, "_absgrad", False):
            r.setAbsgrad(True)          # the backward below adds hypot(W/2 Ax, H/2 Ay) instead (absgrad.py)
        if self.adc is not None and self.iteration <= self.adc.densify_until:
            # the backward below adds the view's statistic (adc.py); behind densify_until no event reads it any more
            r.setADCStats(*self._adcAccumulators())

    def _forwardAndLoss(self, camera, targetRGB, viewKey, lossOut):
        """lossFn of one view (GaussianTrainer.swift:627-723): forward, L1 + DSSIM loss -> lossOut[4] and the colour cotangent
        in self._cot -- with depth= also the depth term and the depth and alpha cotangents; the forward is repeated once if it overflowed on the view's first visit, and once without depth cuts if
        it missed under them."""
        r, m = self.gaussRender, self.model
        wd = self._depthStep is not None or self._normalStep is not None      # (without a depth or normal term the step renders no depth image)
        res = r._measure("train.forward", lambda: r.renderForward(m.getParams(), camera, viewKey=viewKey, wantDepth=wd))
        if viewKey is not None and viewKey not in self._checked_views:
            # first visit of a view: its pair count is unknown -- wait for the forward once and make sure it fitted
            # (rank-local also in a data-parallel job: a forward is no collective, and gs_sync reports whatever the knob says)
            self._checked_views.add(viewKey)
            if self.checkOverflow():
                res = r.renderForward(m.getParams(), camera, viewKey=viewKey, wantDepth=wd)
        r._measure("train.loss.total", lambda: r.lossForwardBackward(res.render, targetRGB, self.lambda_dssim,
                                                                      out=dict(loss=lossOut, cotColor=self._cot),
                                                                      targetKey=self._lossTargetKey(viewKey)))
        self._depthTerms(res, lossOut)
        # depth cuts (renderer.renderForward): nothing that changes state has been queued yet; the loss kernel above
        # keeps the GPU busy while the host learns whether the forward has to be repeated in full
        if viewKey is not None and r.forwardMissed():
            self.forwardMisses += 1
            res = r.renderForward(m.getParams(), camera, viewKey=viewKey, depthCuts=False, wantDepth=wd)
            r.lossForwardBackward(res.render, targetRGB, self.lambda_dssim, out=dict(loss=lossOut, cotColor=self._cot),
                                  targetKey=self._lossTargetKey(viewKey))
            self._depthTerms(res, lossOut)
        if self._distortionStep is not None:       # on the final forward's lists: not in _depthTerms, which runs before the check
            self._distortionLoss(lossOut)

    def _depthTerms(self, res, lossOut):
        """The terms on the render's depth and alpha images, behind the colour loss: the depth term, then the normal term."""
        if self._depthStep is not None:
            self._depthLoss(res, lossOut)
        if self._normalStep is not None:
            self._normalLoss(res, lossOut)

    def _geometryAdam(self, lr: dict, scale: float):
        """Adam on the geometry slice after the all-reduce; the xyz segment's gradient = reduced + the view-direction terms the
        SH kernel rebuilt meanwhile (gs_adam_step_add)."""
        r, m = self.gaussRender, self.model
        _adamStep(r, "gs_adam_step_add", m.geom_numel, (m.arena, m.grad, m.m, m.v), m.seg_end[:4],
                  (lr["xyz"], lr["scales"], lr["rotation"], lr["opacity"]), scale, after=(_p(self._xyz_add), 3 * m.N))

    def _arenaAdam(self, fn: str, scale: float, **kw):
        """Adam over the whole arena, its six segments at the step's learning rates."""
        m = self.model
        _adamStep(self.gaussRender, fn, m.numel, (m.arena, m.grad, m.m, m.v), self._seg_end,
                  arenaLearningRates(self.iteration, self.iterationCount), scale, **kw)

    def _shCompressedUpdate(self, stepCameras, own, scale: float, gather, reduce, xt):
        """The update of a step in the sh_compressed form, one view or several: wait for the gathered colour cotangents, rebuild
        the SH gradients over the step's len(own) views (fuse_adam: with the SH tensors' Adam step in the same pass, on the old
        xyz; own[q]: view q's xyz gradient without its view-direction term where this rank rendered q, else None), wait for the
        geometry slice's all-reduce -- the rebuild ran under it --, then Adam on the geometry slice (fuse_adam) or on the whole
        arena, all at grad_scale `scale`.  gather / reduce: the collectives' Work, None where nothing is to wait for."""
        r, m = self.gaussRender, self.model
        self._awaitGather(gather, xt)
        centres = np.stack([np.asarray(getattr(c, "cameraCenter", c), np.float32).reshape(3) for c in stepCameras])
        if self.fuse_adam:
            lr = dict(zip(PARAM_ORDER, getLearningRates(self.iteration, self.iterationCount)))
            r.shGradFromViewsAdamDir(m.getParams(), self._cc_all, centres, own, m.arena, m.m, m.v, lr["features_dc"],
                                     lr["features_rest"], scale, self._xyz_add)
        else:
            r.shGradFromViews(m.getParams()["xyz"], self._cc_all, centres, m.K, out=m.getGrads())
        if reduce is not None:
            self._xt_mark(xt, "wr0")
            reduce.wait()
            self._xt_mark(xt, "wr1")
        if self.fuse_adam:
            self._geometryAdam(lr, scale)
        else:
            self._arenaAdam("gs_adam_step", scale)

    def _trainStepMulti(self, cameras, targets, stepCameras=None, viewKeys=None):
        """One iteration over viewsPerRank views of this rank (see __init__): cameras / targets / viewKeys are sequences of
        that length, stepCameras the cameras (or centres) of ALL world x V views of the step, rank-major.  Per view: lossFn,
        then the data-parallel backward -- colour cotangents and the view's gate word into the view's block, the four geometry
        gradients into the view's slice, |grad xyz| into the densify statistic -- exactly what a rank of a one-view-per-rank
        job does; then ONE update: geometry slices summed (+ all-reduce), blocks gathered (or simply there), SH gradients
        rebuilt over all views with their Adam step, geometry Adam, both at grad_scale 1 / (world x V)."""
        r, m = self.gaussRender, self.model
        V, N = self.viewsPerRank, m.N
        if len(cameras) != V or len(targets) != V or (viewKeys is not None and len(viewKeys) != V):
            raise ValueError(f"views_per_rank = {V}: trainStep takes {V} cameras, targets and view keys")
        total = self.world * V
        if stepCameras is None and not self._exchange:
            stepCameras = cameras
        if stepCameras is None or len(stepCameras) != total:
            raise ValueError(f"sh_compressed exchange needs stepCameras: {total} cameras (ranks x views_per_rank, rank-major)")
        self._beginIteration()
        ccf = cc_block_floats(N)
        blocks = self._cc_local.view(V, ccf)
        for j in range(V):
            key = None if viewKeys is None else viewKeys[j]
            self._forwardAndLoss(cameras[j], targets[j], key, self._loss_v[j])
            # the view's gate word goes behind ITS block (gs_set_overflow_rider: the word of the last forward)
            r._check(r.lib.gs_set_overflow_rider(r.ctx, C.c_void_p(blocks[j].data_ptr() + 12 * N)))
            if self.fuse_adam:
                r.renderBackwardDPGeom(self._cot, blocks[j], self._geom_views[j], self._xyz_own[j])
            else:
                r.renderBackwardDPBegin(self._cot, colorCot=blocks[j])
                r.renderBackwardDPFinish(out=self._geom_views[j])
            if self.densify:
                self.addGradientAccumulation()
        g_geom = m.grad[:m.geom_numel]
        torch.sum(self._geom_v, dim=0, out=g_geom)               # the rank's share of the all-reduce, summed by addressing
        gather = reduce = None
        xt = self._xt_step() if self._exchange else None
        if self._exchange:
            import torch.distributed as dist
            gather = self._gatherColourCotangents(xt)
            reduce = dist.all_reduce(g_geom, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
            if xt is not None:
                xt["work"].update(reduce=reduce)
        own = None
        if self.fuse_adam:
            own = [None] * total
            for j in range(V):
                own[self.rank * V + j] = self._xyz_own[j]
        self._shCompressedUpdate(stepCameras, own, 1.0 / total, gather, reduce, xt)
        torch.mean(self._loss_v, dim=0, out=self._loss)          # this rank's views; the step's loss is the mean over all of them
        return self._finishIteration()

    def _depthCots(self) -> dict:
        """The backward's depth and alpha cotangents: none without a depth term (the calls are then today's)."""
        if self._depthStep is None and self._normalStep is None:
            return {}
        return dict(cotDepth=self._cotDepth, cotAlpha=self._cotAlpha)

    def _trainStep(self, camera, targetRGB, stepCameras=None, viewKey=None):
        r, m = self.gaussRender, self.model
        self._beginIteration()
        self._forwardAndLoss(camera, targetRGB, viewKey, self._loss)
        xt = None
        if self._gate is not None:
            # (this step's gate: the backward's first kernel stores the forward's overflow word behind what the step's first
            # collective carries -- the word of the LAST forward, i.e. of a forward repeated without depth cuts if there was
            # one; a rank that repeats adds no collective)
            xt = self._xt_step()
        fused = False
        if self._native:
            self._nativeStep(stepCameras)
            fused = True
        elif not self._exchange and self.fuse_adam:
            r._measure("bwd.fused+train.optimizer.applySingle", lambda: r.renderBackwardAdam(
                self._cot, m.arena, m.m, m.v, getLearningRates(self.iteration, self.iterationCount), **self._depthCots()))
            fused = True
        elif not self._exchange:
            r.renderBackward(self._cot, out=m.getGrads(), **self._depthCots())
            if self.mcmc is not None:
                g = m.getGrads()
                r.mcmcRegularizerGrad(m.getParams()["scales"], m.getParams()["opacity"], g["scales"], g["opacity"],
                                      self._mcmcParams())
        elif self.dp_exchange == "allreduce":
            r.renderBackward(self._cot, out=m.getGrads())          # adds this view's |grad xyz| before the sum below
            self._xt_mark(xt, "wr0")                     # (a blocking collective: all of it is exposed)
            allreduce_gradients(m._gbuf[:m.numel + 1], self.pg)      # the arena and, behind it, the step's gate word
            self._xt_mark(xt, "wr1")
        else:
            if stepCameras is None or len(stepCameras) != self.world:
                raise ValueError("sh_compressed exchange needs stepCameras (one camera per rank, rank order)")
            import torch.distributed as dist
            g = m.getGrads()
            # the colour cotangents are ready after the blend backward: their all-gather runs under the projection
            # backward, and the rebuild of the SH gradients under the all-reduce of the geometry slice
            if self.fuse_adam:
                # round 6: no SH rows in the geometry backward (the SH kernel below rebuilds the view-direction term of the xyz
                # gradient and adds the densify statistic), and the colour cotangents + gate word ride in that kernel
                r.renderBackwardDPGeom(self._cot, self._cc_local, g, self._xyz_own[0])
                gather = self._gatherColourCotangents(xt)
            else:
                r.renderBackwardDPBegin(self._cot, colorCot=self._cc_local)      # + this rank's word of the gate at [3 N]
                gather = self._gatherColourCotangents(xt, inline=False)          # (runs under the projection backward below)
                r.renderBackwardDPFinish(out=g)
            reduce = dist.all_reduce(m.grad[:m.geom_numel], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
            if xt is not None:
                xt["work"].update(reduce=reduce)
            own = [self._xyz_own[0] if q == self.rank else None for q in range(self.world)] if self.fuse_adam else None
            self._shCompressedUpdate(stepCameras, own, 1.0 / self.world, gather, reduce, xt)
            fused = True         # (the update is done, Adam included, with or without fuse_adam)
        if self.densify:
            self.addGradientAccumulation()        # (the statistic's denominator: the backward above has added this view's |grad xyz|)
        if not fused and self.sparse_adam:
            # the rows the step's forward saw, and only those (rows >= N of a strided layout and the pads are left alone too)
            widths = (C.c_int * 6)(*[max(int(m._per[k]), 1) for k in ARENA_ORDER])      # (K = 1: an empty segment, any width)
            self._arenaAdam("gs_adam_step_visible", 1.0, before=(widths,), after=(m.N, None))
        elif not fused:
            self._arenaAdam("gs_adam_step", 1.0 / self.world)
            if self.mcmc is not None:
                p = m.getParams()
                r.mcmcInjectNoise(p["xyz"], p["scales"], p["rotation"], p["opacity"],
                                  getLearningRates(self.iteration, self.iterationCount)[0], self._mcmcParams())
        for t in self._perView.values():
            t.adam(r, int(viewKey), self.iteration, self.iterationCount)
        return self._finishIteration()

    def _finishIteration(self):
        r, m = self.gaussRender, self.model
        it = self.iteration
        self.iteration += 1
        if self.outputDirectory is not None and it % self.save_snapshot_per_iteration == 0:
            self.save_snapshot(it)
        if self.mcmc is not None and self.mcmc.is_event(it):
            self._mcmcEvent(it)
            # the event has just waited for the device (its count reads): the overflow flag is cheap to look at now
            if self._overflow_reported():
                self.checkOverflow()
        if self.adc is not None:
            if self.adc.is_event(it):
                self._adcEvent(it)
                # the event has just waited for the device (its count read): the overflow flag is cheap to look at now
                if self._overflow_reported():
                    self.checkOverflow()
            if self.adc.is_reset(it):
                self._adcResetOpacity()
        moved = False         # (filter_3d: the model's rows or positions changed other than by the step)
        if self.densify and it % self.split_and_prune_per_iteration == 0:
            self._committed = False
            self.split_and_prune(it)
            moved = self._committed
            # the reference re-creates the optimizer state after every call, changed or not (:1098-1110); a committed
            # event has just done so (GaussModel.commitStaged)
            if not self._committed:
                m.resetOptimizerState()
                if self.referenceParamReload and self._committed_params is not None \
                        and self._committed_params.numel() == m.arena.numel():
                    m.arena.copy_(self._committed_params)      # `params = model.getParams()` (:1100): the last COMMITTED tensors
                    moved = True
            # the event has just waited for the device (its .item()): the overflow flag is cheap to look at now, and in a
            # data-parallel job every rank is here at the same iteration
            if self._exchange and not self._plans_events():
                self._collectiveOverflowCheck(force=self._committed)
            elif self._exchange:
                pass        # a planned event has not drained the queue: the ranks look together at the next cadence (every overflowCheckInterval steps)
            elif self._overflow_reported():
                self.checkOverflow()
        if self.contribPrune is not None and self.contribPrune.is_event(it):
            self._contribPruneEvent(self.contribPrune.cameras, self.contribPrune.threshold, self.contribPrune.score)
            moved = moved or self._committed
        if self.filter_3d and (moved or self.iteration % self.filter3dInterval == 0):
            self._updateFilter3D()        # for the new N, before the next forward
        return self._loss
