"""Progressive SH degree: training starts at a low active degree and adds a band at a time (include/gsplat.h gs_set_sh_degree,
DESIGN.md section 30; Inria's oneupSHdegree every 1000 iterations, gsplat's sh_degree_interval).

    degree_at(t) = min(cap, start + t // every)

with t the trainer's iteration counter from 0 and cap = max_degree, or the renderer's maximum where max_degree is None.  The
schedule holds no state: GaussianTrainer(sh_schedule=...) asks it before every step and never lowers the degree during a run.
"""
from __future__ import annotations


def active_columns(degree: int) -> int:
    """Lact = 3 ((degree + 1)^2 - 1): the columns of a features_rest row (flattened [K - 1, 3]) that degree `degree` reads."""
    degree = int(degree)
    if degree < 0:
        raise ValueError("active_columns: degree >= 0")
    return 3 * ((degree + 1) ** 2 - 1)


class SHDegreeSchedule:
    def __init__(self, start: int = 0, every: int = 1000, max_degree: int | None = None):
        self.start, self.every, self.max_degree = start, every, max_degree
        self.validate()

    def validate(self):
        for name, v, lo in (("start", self.start, 0), ("every", self.every, 1)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"SHDegreeSchedule: {name} is an integer >= {lo}")
        m = self.max_degree
        if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 0):
            raise ValueError("SHDegreeSchedule: max_degree is None or an integer >= 0")

    def degree_at(self, iteration: int, renderer_max: int | None = None) -> int:
        """The active degree of step `iteration` (0-based); renderer_max: the renderer's maxSHDegree, the cap where max_degree
        is None and a bound on it otherwise."""
        if iteration < 0:
            raise ValueError("SHDegreeSchedule.degree_at: iteration >= 0")
        d = self.start + int(iteration) // self.every
        for cap in (self.max_degree, renderer_max):
            if cap is not None:
                d = min(d, int(cap))
        return d

    def __repr__(self):
        return f"SHDegreeSchedule(start={self.start}, every={self.every}, max_degree={self.max_degree})"
