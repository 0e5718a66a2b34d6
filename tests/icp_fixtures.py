"""Seeded clouds for the ICP tests, each named for the branch it reaches.  Coordinates sit about 10 m from the origin, so
a float32 coordinate is rounded by up to 2^-21 m ~ 5e-7 m."""
import functools

import numpy as np

import icp_numpy as ref

f32 = np.float32
KNOWN_RVEC = np.array([0.01, -0.02, 0.015])  # x0, x1, x2 of Rz(x2) Ry(x1) Rx(x0)
KNOWN_T = np.array([0.05, -0.03, 0.04])


def known_pose():
    """the pose the corner source was moved by: T maps the source back onto the target"""
    T = np.eye(4)
    T[:3] = ref.update_matrix(np.r_[KNOWN_RVEC, KNOWN_T])
    return T


def _patch(axis, m, seed, lo=12.0, step=0.25, level=10.0):
    """m x m jittered lattice on the plane `axis` = level; the patch starts 2 m from the corner's edges, further than any
    30-neighbour radius, so every neighbourhood lies in one plane"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    uv = lo + step * np.stack([u.ravel(), v.ravel()], 1) + rng.uniform(-0.05, 0.05, (m * m, 2))
    p = np.full((m * m, 3), level)
    p[:, [a for a in range(3) if a != axis]] = uv
    return p


def corner(n, seed=1, step=0.25):
    """three mutually perpendicular planes (a corridor corner) on jittered lattices, n points in a seeded order"""
    m = int(np.ceil(np.sqrt(n / 3.0)))
    p = np.concatenate([_patch(a, m, seed + a, step=step) for a in range(3)])
    return p[np.random.default_rng(seed + 7).permutation(len(p))[:n]].astype(f32)


def corner_source(n, seed=11):
    """other samples of the same three planes, moved by the inverse of known_pose() and rounded to float32"""
    m = int(np.ceil(np.sqrt(n / 3.0)))
    p = np.concatenate([_patch(a, m, seed + a) for a in range(3)])
    p = p[np.random.default_rng(seed + 7).permutation(len(p))[:n]]
    Ti = np.linalg.inv(known_pose())
    return (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)


def _case(tgt, src, max_dist, T=None, knn=30, pair=(15.0, 1.5)):
    return dict(tgt=np.ascontiguousarray(tgt, f32), src=np.ascontiguousarray(src, f32), max_dist=max_dist,
                T=np.eye(4) if T is None else T, knn=knn, pair=pair)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(tgt, src, max_dist, T, knn, pair)"""
    rng = np.random.default_rng(3)
    out = {}
    # the corner pair: 1200 target points (19 level-1 boxes), 300 source points, found from the identity
    out["corner_pair"] = _case(corner(1200), corner_source(300), 15.0)
    # one past two box fan-outs (4097 = 64 * 64 + 1: a second level-2 box), 65 source points, started at the known pose
    out["corner_4097"] = _case(corner(4097, step=0.125), corner_source(65), 1.5, T=known_pose())
    # exact duplicates: the last 20 target points repeat the first 20, the source is those 20 points three times over and
    # five more (65): d2 = 0 ties that the lower index must win
    t = corner(45)
    t = np.concatenate([t, t[:20]])
    out["duplicates"] = _case(t, np.concatenate([t[:20], t[:20], t[:20], t[20:25]]), 1.5, knn=8)
    # a source wholly beyond max_dist: no correspondence, identity update, stop after one iteration
    out["far"] = _case(corner(64), corner(65, seed=5) + f32(40.0), 1.5, pair=(15.0, 1.5))
    # a single plane z = 10: J^T J has three exactly zero columns, so the update is the identity
    pl = _patch(2, 8, 21).astype(f32)
    out["plane"] = _case(pl[:63], (_patch(2, 9, 22)[:65] + [0.02, -0.01, 0.3]).astype(f32), 1.5)
    # collinear points: a covariance of rank one
    s = np.linspace(0.0, 3.0, 64)[:, None]
    line = (np.array([10.0, 11.0, 12.0]) + s * np.array([1.0, 2.0, -1.0])).astype(f32)
    out["collinear"] = _case(line, (line[:1] + f32(0.01)), 1.5, knn=5)
    # one and two target points: every list is short, every normal is (0, 0, 1)
    out["n_tgt_1"] = _case(corner(1), corner(1) + f32(0.1), 1.5, knn=3)
    out["n_tgt_2"] = _case(corner(2), corner_source(65), 15.0, knn=3)
    # 65 target points: one past the first fan-out; unstructured, the source a noisy copy
    c = (10.0 + rng.uniform(0, 3, (65, 3))).astype(f32)
    out["n_tgt_65"] = _case(c, (c[rng.permutation(65)][:65] + rng.normal(0, 0.02, (65, 3))).astype(f32), 1.5, knn=30)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything the restatement computes for a case, once"""
    c = cases()[name]
    tgt, src, T, md = c["tgt"], c["src"], c["T"], c["max_dist"]
    r = dict(rec=ref.new_record())
    r["knn"] = ref.knn(tgt, c["knn"])
    r["cnt"], r["cov"] = ref.covariance(tgt, r["knn"])
    r["normals"] = ref.normals_from_covariance(r["cnt"], r["cov"])
    pcd = ref.move(T, src.astype(np.float64))
    r["corr"], _, r["fitness"], r["rmse"] = ref.evaluate(pcd, tgt, md, r["rec"])
    r["JtJ"], r["Jtr"], r["n_corr_step"] = ref.normal_equations(src, tgt, r["normals"], md, T)
    r["icp"] = ref.icp(src, tgt, r["normals"], md, T, rec=r["rec"])
    r["info"], r["n_corr"], r["info_corr"] = ref.information(src, tgt, md, T)
    r["pair"] = ref.pairwise(src, tgt, r["normals"], *c["pair"])
    return r
