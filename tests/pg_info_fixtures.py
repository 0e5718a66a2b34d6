"""Weighted pose graphs for the information-matrix tests: the drifting-loop chains of pg_fixtures with seeded sets of
information matrices, and a square lap whose end is offset from its start by a known transform."""
import numpy as np
from scipy.spatial.transform import Rotation as Rot

from pg_fixtures import drifting_loop, pose7

TRIU = np.triu_indices(6)

# (vertices, closures (at, to)): ne = 40, one partial workgroup of the linearisation; ne = 131, a second workgroup whose
# tail threads redo the last edge; 313 vertices, closure endpoints inside and at the end of the 104-row segments
GRAPHS = {40: [(39, 0)], 130: [(128, 3), (129, 0)], 313: [(200, 50), (312, 0)]}


# The closures are identity measurements between vertices a few steps apart: a large-residual problem on which plain
# Gauss-Newton (no damping, as the reference runs it) converges only while that mismatch is small, and the tests' bounds
# rest on cond(H) eps ~ 1e5 * 1e-16 at 313 vertices.  The generator's parameters were chosen ON THE CPU, with the arbiter
# alone (chi2 per iteration and numpy.linalg.cond of its H, unweighted graph):
#   defaults (radius 20 m, one lap): chi2 GROWS from the second iteration on at 130 vertices (128 -> 3 and 129 -> 0
#       contradict each other by four steps = 3.9 m) and at 313 (200 -> 50 is a chord across the circle);
#   313 vertices as 2.05 laps of 153 (both closures then join vertices within six steps): converges, but on the 20 m circle
#       cond(H) = 1.9e9 (1.0e10 with set d) -- four decades from the 1e5 the bounds assume; a single float64 Cholesky of the
#       arbiter's own system, in any elimination order, is then at 2e-10 ... 7e-10 and the comparison measures conditioning;
#   a 0.5 m circle (steps of 2 ... 8 cm, rotation per step unchanged): cond(H) = 2.0e3 / 2.6e4 / 1.0e5 at 40 / 130 / 313
#       vertices (1.4e5 / 1.5e6 / 5.6e6 with set d), and the arbiter's chi2 falls monotonically for the unweighted graph and
#       the sets s, d and f.
PARAMS = {40: dict(radius=0.5), 130: dict(radius=0.5), 313: dict(radius=0.5, laps=313 / 153)}


def chain(V):
    """-> (estimates [V, 7], closures) of the drifting loop with V vertices"""
    gt, est = drifting_loop(V, yaw_drift=1e-3, **PARAMS[V])
    return np.array(est), GRAPHS[V]


def edge_list(est, closures):
    """the edges in the order augment_node / add_loop_closure create them: (from, to, is_closure)"""
    out = []
    for i in range(1, len(est)):
        out.append((i - 1, i, False))
        for at, to in closures:
            if at == i:
                out.append((i, to, True))
    return out


def omega_set(kind, edges, seed=5):
    """One 6 x 6 information matrix per edge.  s: 4 I everywhere; d: diag(100,100,100,1,1,1) on odometry edges and
    diag(1,1,1,100,100,100) on closures; f: Q diag(lambda) Q^T per edge, Q from the QR of a seeded Gaussian matrix,
    lambda log-uniform in [1, 100]."""
    rng = np.random.default_rng(seed)
    out = []
    for (_, _, closure) in edges:
        if kind == "s":
            out.append(4.0 * np.eye(6))
        elif kind == "d":
            out.append(np.diag([1, 1, 1, 100, 100, 100.0] if closure else [100, 100, 100, 1, 1, 1.0]))
        elif kind == "f":
            Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            M = Q @ np.diag(10.0 ** rng.uniform(0, 2, 6)) @ Q.T
            out.append((M + M.T) / 2)
        else:
            raise ValueError(kind)
    return out


def tri21(M):
    return np.ascontiguousarray(np.asarray(M, np.float64)[TRIU])


def _inv7(p):
    R = Rot.from_quat(p[3:]).as_matrix()
    return pose7(R.T, -R.T @ p[:3])


def _mul7(a, b):
    Ra, Rb = Rot.from_quat(a[3:]).as_matrix(), Rot.from_quat(b[3:]).as_matrix()
    return pose7(Ra @ Rb, a[:3] + Ra @ b[:3])


def square_lap(n=40, side=10.0, drift_seed=0, yaw_sigma=4e-3):
    """A square lap of n poses in the x-z plane whose last pose is offset from pose 0 by a known T (0.4 m, 5 degrees);
    odometry = the true relative motions with a seeded yaw drift per step.
    -> (gt [n, 7], est [n, 7], meas7 = X_{n-1}^-1 X_0 of the ground truth)"""
    rng = np.random.default_rng(drift_seed)
    per = n // 4
    gt = []
    for k in range(n):
        s, u = divmod(k, per)
        corner = np.array([[0, 0, 0], [0, 0, side], [side, 0, side], [side, 0, 0]], float)[s]
        head = np.array([[0, 0, 1], [1, 0, 0], [0, 0, -1], [-1, 0, 0]], float)[s]
        yaw = -np.pi / 2 * s  # heading along +z, then +x, -z, -x
        gt.append((Rot.from_euler("y", -yaw).as_matrix(), corner + head * side * u / per))
    # the last pose: pose 0 composed with the known offset T
    T_R = Rot.from_euler("y", np.deg2rad(5.0)).as_matrix()
    T_t = np.array([0.4, 0.0, 0.0]) @ Rot.from_euler("y", 0.3).as_matrix().T
    gt[-1] = (gt[0][0] @ T_R, gt[0][1] + gt[0][0] @ T_t)
    gt7 = np.array([pose7(R, t) for R, t in gt])
    est = [gt[0]]
    for i in range(1, n):
        Rrel = gt[i - 1][0].T @ gt[i][0]
        trel = gt[i - 1][0].T @ (gt[i][1] - gt[i - 1][1])
        Rrel = Rrel @ Rot.from_euler("y", rng.normal(0, yaw_sigma)).as_matrix()
        est.append((est[-1][0] @ Rrel, est[-1][1] + est[-1][0] @ trel))
    est7 = np.array([pose7(R, t) for R, t in est])
    meas = _mul7(_inv7(gt7[-1]), gt7[0])
    if meas[6] < 0:
        meas[3:] = -meas[3:]
    return gt7, est7, meas


def rms_translation(X, gt):
    return float(np.sqrt(np.mean(np.sum((X[:, :3] - gt[:, :3]) ** 2, axis=1))))
