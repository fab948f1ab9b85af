"""The p / q schedule of LpqLoss (LpqLossParameter, caffe.proto:584-601): episodes that start at given solver iterations."""
from __future__ import annotations

from typing import Sequence, Tuple


class LpqSchedule:
    """(pq_episode_starts_at_iter, p, q) with the checks and messages of LpqLossLayer::LayerSetUp (lpq_loss_layer.cpp:19-82):
    one p and one q without a start are constant parameters; otherwise the three lists have the same, non-zero size, the starts increase
    strictly and the first one is 0.  A failed check raises ValueError (layers.CheckError is one) with the reference's LOG(FATAL) text.

    at(iter) -> (p, q) is a pure function of the iteration: the episode with the largest start not above `iter`.  The reference pops a
    queue in Forward_gpu (lpq_loss_layer.cu:100-135) and so never steps back once an episode has been left; for the non-decreasing
    iterations of a solver run the two agree, and a net that is evaluated at an earlier iteration gets that iteration's episode here."""

    def __init__(self, starts: Sequence[int] = (), ps: Sequence[float] = (), qs: Sequence[float] = (), error=ValueError):
        starts, ps, qs = [int(s) for s in starts], [float(p) for p in ps], [float(q) for q in qs]
        if len(starts) == 0 and len(ps) == 1 and len(qs) == 1:
            starts = [0]                                                                       # cpp:29-37
        else:
            if len(starts) != len(ps) or len(ps) != len(qs):                                   # cpp:41-47
                raise error("Incompatible sizes: (pq_episode_starts_at_iter -> %d, p -> %d, q -> %d)" % (len(starts), len(ps), len(qs)))
            if len(starts) < 1:                                                                # cpp:49-51
                raise error("Lpq schedule parameters must not be empty")
            for i in range(len(starts) - 1):                                                   # cpp:53-64
                if starts[i] >= starts[i + 1]:
                    raise error("pq_episode_starts_at_frame is not ordered or contains duplicates:" + "".join(" %d" % s for s in starts))
            if starts[0] != 0:                                                                 # cpp:66-69
                raise error("First entry in pq_episode_starts_at_frame is not 0, this is probably a mistake.")
        self.starts, self.ps, self.qs = tuple(starts), tuple(ps), tuple(qs)

    def step(self, iteration: int) -> int:
        """Index of the episode in force at `iteration` (fn2_lpq_loss_schedule_step computes the same)."""
        k = 0
        for i, s in enumerate(self.starts):
            if s <= int(iteration):
                k = i
        return k

    def at(self, iteration: int) -> Tuple[float, float]:
        k = self.step(iteration)
        return self.ps[k], self.qs[k]

    def __len__(self):
        return len(self.starts)

    def __repr__(self):
        return "LpqSchedule(starts=%r, ps=%r, qs=%r)" % (self.starts, self.ps, self.qs)
