"""The collectives over the trait-shard ranks: the one owner of torch.distributed in the package.

A RankGroup decides once where tensors are staged -- on the host for gloo (tests on a one-GPU box), else on the device
of the handle it serves (RCCL) -- and offers exactly the exchanges the sharded paths of core.VbRun and postproc.fdr_cutoff
need.  Every method is a collective: all ranks call the same ones in the same order.
"""
from __future__ import annotations

import numpy as np


class RankGroup:
    def __init__(self, process_group, device):
        import torch
        import torch.distributed as dist
        self._torch, self._dist = torch, dist
        self.pg = process_group
        self.rank = dist.get_rank(process_group)
        self.world = dist.get_world_size(process_group)
        self.device = torch.device("cuda", int(device))          # the handle's device, not torch's current one
        self.host_staged = dist.get_backend(process_group) == "gloo"
        self._stage = torch.device("cpu") if self.host_staged else self.device

    def _staged(self, a):
        return self._torch.from_numpy(np.array(a)).to(self._stage)       # a copy: the caller's array is left as it is

    def sum(self, a):
        """A numpy array of any shape, int64 or float64, summed over the ranks: same shape and dtype."""
        t = self._staged(a)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self.pg)
        return t.cpu().numpy()

    def max(self, v):
        t = self._staged(np.array([float(v)]))
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX, group=self.pg)
        return float(t.item())

    def gather(self, a):
        """A small array of the same shape and dtype on every rank, from every rank: a list in rank order."""
        t = self._staged(a)
        outs = [self._torch.zeros_like(t) for _ in range(self.world)]
        self._dist.all_gather(outs, t, group=self.pg)
        return [o.cpu().numpy() for o in outs]

    def sum_in_rank_order(self, v):
        """Sum of one double per rank, added in rank order on every rank: the same bits everywhere (an all-reduce may add
        in another order on another rank)."""
        total = 0.0
        for part in self.gather(np.array([float(v)])):
            total += float(part[0])
        return total

    def gather_rows(self, rows):
        """Every rank's (m, 4) float64 table, m its own, on every rank as a list in rank order: one gather of the counts,
        one of the rows padded to the longest table (int32 indices travel as doubles, exactly)."""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
        counts = [int(c[0]) for c in self.gather(np.array([len(rows)], dtype=np.int64))]
        buf = np.zeros((max(max(counts), 1), 4))
        buf[:len(rows)] = rows
        return [o[:c] for o, c in zip(self.gather(buf), counts)]

    def device_zeros(self, n):
        """A float64 payload buffer on the handle's device (aq_vb_reduce_len(p) doubles, or 8)."""
        return self._torch.zeros(int(n), dtype=self._torch.float64, device=self.device)

    def allreduce_device(self, t):
        """In-place SUM of a device tensor -- the per-sweep payload.  RCCL reduces the device buffer where it is; gloo
        stages it through the host."""
        if self.host_staged:
            h = t.cpu()
            self._dist.all_reduce(h, op=self._dist.ReduceOp.SUM, group=self.pg)
            t.copy_(h)
        else:
            self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self.pg)
