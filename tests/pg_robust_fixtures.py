"""Graphs for the robust-kernel tests, chosen ON THE CPU with the arbiter alone (tests/pg_info_arbiter.py through
tests/pg_robust_numpy.py): the 0.5 m drifting loops of pg_info_fixtures at 40 and 130 vertices with their true closures, and the
130-vertex one with one FALSE closure, 90 -> 20 with the identity measurement (two vertices 0.9 m and 190 degrees apart).

What the arbiter's re-weighted Gauss-Newton gives on them (tests/test_pg_robust_numpy.py asserts all of it):
  * no kernel: the false edge takes rms_translation against the generator's poses from 0.039 m to 0.50 m (12.7 x);
  * Geman-McClure, mu = 0.03, on the three closures, ten iterations: the false edge ends at w = 2.5e-4 (identity information) and
    9e-8 (set d), the true closures at w >= 0.96 and >= 0.86.  (mu = 0.01 with set d, and mu = 0.003 with either, lose the closure
    128 -> 3 as well: its identity measurement contradicts the odometry by four steps, chi2 = 0.065 at the start.)
  * KERNELS below, on EVERY edge, four iterations: no chi2 within 1e-6 relative of a Huber or DCS branch point, and cond(H) of the
    re-weighted system stays below the 5.6e6 of DESIGN.md section 10g."""
import functools

import numpy as np

import pg_robust_numpy as rn
from pg_fixtures import drifting_loop, pose7
from pg_info_fixtures import PARAMS, _inv7, _mul7, chain, edge_list, omega_set

ID7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
FALSE_CLOSURE = (90, 20)
MU = 0.03                    # Geman-McClure on the closures of the false-closure graph
PRUNE_THRESHOLD = 0.25
# the parameter of each kind for the per-iteration tests (kernels on every edge).  chi2 of the closures at the start is 0.016 ... 0.065
# (true) and 2.0 (false), of the odometry edges 0: every kind has edges on either side of its branch point.
KERNELS = {rn.HUBER: 0.1, rn.CAUCHY: 0.2, rn.DCS: 0.02, rn.GEMAN_MCCLURE: 0.03}
CASES = ("40", "130", "130f")


@functools.lru_cache(maxsize=None)
def graph(name):
    """name: "40", "130" or "130f" (with the false closure)
    -> (est [V, 7], closures [(at, to)], edge list [(from, to, is_closure)], edges [(from, to, Z7)], gt [V, 7])"""
    V = int(name.rstrip("f"))
    est, closures = chain(V)
    closures = list(closures) + ([FALSE_CLOSURE] if name.endswith("f") else [])
    el = edge_list(est, closures)
    edges = [(i, j, ID7.copy() if c else _mul7(_inv7(est[i]), est[j])) for (i, j, c) in el]
    gt = np.array([pose7(R, t) for R, t in drifting_loop(V, yaw_drift=1e-3, **PARAMS[V])[0]])
    return est, closures, el, edges, gt


def false_edge_index():
    el = graph("130f")[2]
    return next(k for k, (i, j, c) in enumerate(el) if c and (i, j) == FALSE_CLOSURE)


def closure_indices(name):
    return [k for k, (_, _, c) in enumerate(graph(name)[2]) if c]


@functools.lru_cache(maxsize=None)
def omegas(name, kind):
    """kind: "i" (identity everywhere: None) or "d" (omega_set('d'))"""
    return None if kind == "i" else tuple(omega_set(kind, graph(name)[2]))


def kernels_on_closures(name, kind=rn.GEMAN_MCCLURE, delta=MU):
    return [(kind, delta) if c else None for (_, _, c) in graph(name)[2]]


def kernels_everywhere(name, kind):
    return [(kind, KERNELS[kind])] * len(graph(name)[2])


def branch_margin(kind, delta, c):
    """the smallest relative distance of a chi2 from the kind's branch point (inf for the kinds that have none)"""
    c = np.asarray(c, np.float64)
    if kind == rn.HUBER:
        return float(np.min(np.abs(c - delta * delta)) / (delta * delta))
    if kind == rn.DCS:
        return float(np.min(np.abs(c - delta)) / delta)
    return float("inf")


@functools.lru_cache(maxsize=None)
def gm_run(name, om_kind, iters=10):
    """The arbiter's re-weighted Gauss-Newton with Geman-McClure(MU) on the closures from the fixture's estimates -> list of iterates"""
    est, _, _, edges, _ = graph(name)
    return rn.irls(est, edges, omegas(name, om_kind), kernels_on_closures(name), iters)[1]


def without_edge(seq, k):
    return [x for n, x in enumerate(seq) if n != k]
