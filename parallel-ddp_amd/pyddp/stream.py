"""A handle as a continuously fed solver: more problems than slots, finished slots refilled between sweeps (pddp_load_problems / pddp_store_problems).

SlotScheduler holds the bookkeeping -- which problem sits in which slot, which slots are padding -- and needs only four methods of a solver: status(), iterate(sweeps),
load_problems(idx, x0, u0, xGoal, ignore_first_defect) and store_problems(idx), plus load(x0, u0, xGoal) for the first fill; tests drive it with a fake solver on the CPU.
A stream whose problems carry cost records also needs set_cost_problems(idx, w) and get_cost_problems(idx) -- or, on a solver whose has_diag_cost() is true (pendulum,
cart-pole, quadrotor), set_diag_cost_problems / get_diag_cost_problems; a stream of plain (x0, u0, xGoal) never calls them.
"""
import numpy as np


class SlotScheduler:
    """problems: an iterable of (x0, u0, xGoal), each one problem's arrays ([N][n], [N][m], [n], any shape with those sizes).  run() yields (problem index, result) in the
    order the problems finish; result = that problem's row of store_problems() plus done / iters.
    A problem may be (x0, u0, xGoal, cost_record): its own cost weights (Solver.set_cost_problems: 5 or 9 numbers of the arm; Solver.set_diag_cost_problems: the diagonal
    record of the pendulum, cart-pole or quadrotor), written for its slot immediately before the load
    that puts it there.  Once any problem of the stream has carried a record, a problem without one gets the handle-wide record written for its slot -- a slot never
    inherits its previous tenant's weights."""

    def __init__(self, solver, problems, batch, sweeps_per_poll=4, ignore_first_defect=1):
        self.s, self.it, self.B = solver, iter(problems), int(batch)
        self.sweeps, self.ifd = max(1, int(sweeps_per_poll)), ignore_first_defect
        self.owner = [None] * self.B          # slot -> index of the problem it holds; None: padding or already collected
        self.taken = 0                        # problems drawn from the iterator so far
        self.wide = None                      # the handle-wide cost record, read once before the first per-problem write; None: no problem has carried a record yet

    def _draw(self, limit):
        got = []
        for _ in range(limit):
            try:
                got.append(next(self.it))
            except StopIteration:
                break
        return got

    @staticmethod
    def _stack(probs, k):
        return np.concatenate([np.asarray(p[k]).ravel() for p in probs])

    def _set_costs(self, slots, probs):
        """the cost records of the problems about to be loaded into `slots` (nothing while the stream has carried none)"""
        diag = getattr(self.s, "has_diag_cost", None)
        diag = bool(diag and diag())                               # the diagonal record of plants 1-3, or the arm's record
        if self.wide is None:
            if not any(len(p) > 3 and p[3] is not None for p in probs):
                return
            getter = self.s.get_diag_cost_problems if diag else self.s.get_cost_problems
            self.wide = np.array(getter([0]), dtype=np.float64).reshape(-1)
        w = np.stack([np.asarray(p[3], dtype=np.float64).reshape(-1) if len(p) > 3 and p[3] is not None else self.wide for p in probs])
        (self.s.set_diag_cost_problems if diag else self.s.set_cost_problems)(list(slots), w)

    def run(self):
        first = self._draw(self.B)
        if not first:
            return
        for slot in range(len(first)):
            self.owner[slot] = slot
        self.taken = len(first)
        fill = first + [first[0]] * (self.B - len(first))          # a short stream: the empty slots solve copies of the first problem, whose results are dropped
        self._set_costs(range(self.B), fill)
        self.s.load(self._stack(fill, 0), self._stack(fill, 1), self._stack(fill, 2), clear_vars=1, ignore_first_defect=self.ifd)
        while any(o is not None for o in self.owner):
            self.s.iterate(self.sweeps)
            done, iters = self.s.status()
            ready = [slot for slot in range(self.B) if self.owner[slot] is not None and done[slot]]
            if not ready:
                continue
            rows = self.s.store_problems(ready)
            results = [(self.owner[slot], dict({k: v[j] for k, v in rows.items()}, done=int(done[slot]), iters=int(iters[slot]))) for j, slot in enumerate(ready)]
            fresh = self._draw(len(ready))
            for slot in ready:
                self.owner[slot] = None
            if fresh:
                into = ready[: len(fresh)]
                for j, slot in enumerate(into):
                    self.owner[slot] = self.taken + j
                self.taken += len(fresh)
                self._set_costs(into, fresh)
                self.s.load_problems(into, self._stack(fresh, 0), self._stack(fresh, 1), self._stack(fresh, 2), self.ifd)
            for item in results:
                yield item


def solve_stream(solver, problems, sweeps_per_poll=4, ignore_first_defect=1):
    """Generator: every problem of `problems` (an iterable of (x0, u0, xGoal) or (x0, u0, xGoal, cost_record)) through `solver`'s slots.  The handle is filled with pddp_load (padded with copies of the
    first problem when fewer than `batch` are given; their results are dropped), then iterated sweeps_per_poll sweeps at a time; finished slots are stored, refilled from
    the iterator and yielded as (problem index, result).  Ends when every problem has been yielded."""
    return SlotScheduler(solver, problems, solver.cfg.batch, sweeps_per_poll, ignore_first_defect).run()
