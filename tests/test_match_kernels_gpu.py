"""-m gpu: the single-map matching kernels behind lama::Loc2D, MatchSurface2D / Solve and global localisation (k_match_eval and its
cell mode, k_match_solve_batch as the single solves run it, k_eval_batch, k_sample_likelihood) against the CPU oracle across scan sizes: shorter than
a wave, than a block, tails past the 256-thread block and the 1280-beam gather batch, the point counts for which Loc2D's sampling
step asks for more than 128 terms, on both sides of the LDS sqrt table (max_sqdist 484 / 529) and in the wide library.

Every tolerance and its derivation is in tests/_match_checks.py: per-beam outputs bit-equal (parity tolerances only at poses whose
rotation comes from OCML's trig), sums within n * eps * sum|term| of the exactly rounded sum, sampled likelihoods within
(nterms + 3) * eps, poses within test_gpu_parity.POSE_TOL with identical iteration counts.
"""
import math

import numpy as np
import pytest

import _match_checks as M
import _oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 129, 180, 199, 200, 255, 256, 257, 299, 385, 399, 1080, 1279, 1280, 1281, 2561, 5000]


@pytest.fixture(scope="module")
def F():
    import iris_lama_amd.ffi as f
    if f.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need the MI355X box (there is no CPU fallback)")
    return f


@pytest.fixture(scope="module")
def world(F):
    ctx, dm = M.build_world(F, 1.0)
    yield ctx, dm
    ctx.close()


def _start():
    x, y, yaw = M.SCAN_POSE
    return O.se2(x, y + 0.06, yaw - 0.02)


@pytest.mark.parametrize("n", SIZES)
def test_eval_batch_solve_and_sampling_across_scan_sizes(world, n):
    ctx, dm = world
    pts = M.scan_of(n)
    assert len(pts) == n
    for pose in M.eval_poses(n_rotated=2):
        M.check_eval(ctx, dm, pts, pose, what=n)
    rng = np.random.default_rng(n)
    M.check_batch(ctx, dm, pts, M.batch_poses(rng, 1), what=(n, "B = 1"))
    M.check_batch(ctx, dm, pts, M.batch_poses(rng, 3000), what=(n, "B = 3000"))
    M.check_solve(ctx, dm, pts, _start(), what=(n, "from a perturbed pose"))
    M.check_solve(ctx, dm, pts, O.se2(1.3, 1.65, 0.0), what=(n, "from heading 0"))
    x, y, yaw = M.SCAN_POSE
    xy = [(x, y), (x + 0.05, y - 0.1), (x - 0.3, y + 0.2), (37.0, 2.0), (350.0, -350.0)]
    nterms = M.check_sampling(ctx, dm, pts, yaw, xy, what=n)
    assert nterms <= 256 and nterms == -(-n // max(n // 100, 1))


def test_hits_on_cell_edges(world):
    """mu = 0: the bilinear weights of every hit are exactly 0 (residuals, Jacobian, evaluation-only solve sums bit-exact)"""
    ctx, dm = world
    pts, pose = M.edge_scan()
    hits = pts[:, :2] + pose[2:]
    assert np.all(hits * 20.0 == np.round(hits * 20.0))
    M.check_eval(ctx, dm, pts, pose, what="mu = 0")
    M.check_batch(ctx, dm, pts, pose[None], what="mu = 0")
    M.check_solve(ctx, dm, pts, pose, what="mu = 0")


@pytest.mark.parametrize("mount", sorted(M.MOUNTS))
@pytest.mark.parametrize("n", [65, 257, 1281])
def test_mounted_sensors(world, mount, n):
    """non-zero sensor origin, a yawed mount and an upside-down one (roll pi): eval and solve"""
    ctx, dm = world
    pts, origin, quat = M.mounted_scan(n, M.MOUNTS[mount])
    for pose in M.eval_poses(n_rotated=1):
        M.check_eval(ctx, dm, pts, pose, origin, quat, what=(mount, n))
    M.check_batch(ctx, dm, pts, M.batch_poses(np.random.default_rng(n), 64), origin, quat, what=(mount, n))
    M.check_solve(ctx, dm, pts, _start(), origin, quat, what=(mount, n))


@pytest.mark.parametrize("l2_max,sqdist,bigsq,wide", [(1.1, 484, False, False), (1.12, 529, True, False), (7.0, 19600, True, True)])
def test_lut_and_bigsq_instantiations(F, l2_max, sqdist, bigsq, wide):
    """max_sqdist <= SM_LUT = 512 reads sqrt(sqdist) from the LDS table, above it the BIGSQ instantiations take the square root;
    l2_max = 7 m runs the wide library"""
    cells = math.ceil(l2_max * (1.0 / 0.05))
    assert cells * cells == sqdist and (sqdist > 512) == bigsq and F.needs_wide(l2_max, 0.05) == wide
    ctx, dm = M.build_world(F, l2_max)
    try:
        assert ctx.L is F.hip_lib(wide=wide)
        for n in (1, 65, 257, 1281, 5000):
            pts = M.scan_of(n)
            M.check_batch(ctx, dm, pts, M.batch_poses(np.random.default_rng(n), 300), what=(l2_max, n))
            M.check_solve(ctx, dm, pts, _start(), what=(l2_max, n))
    finally:
        ctx.close()


def test_loc2d_sampling_covariance_at_scan_sizes_that_exceeded_128_terms(F):
    """lama::Loc2D with cov_blend > 0 against the oracle: before SL_MAX_TERMS became 256, scans of 180, 199, 290 and 390 points
    (step = max(n / 100, 1) asks for 180, 199, 145 and 195 terms) were refused by lama_hip_map_sample_likelihood"""
    from _worlds import open_corridor
    obst = open_corridor()
    o = O.Loc(cov_blend=0.35)
    dm = o.dm()
    for x, y in obst:
        c = O.w2m([x, y, 0.0])
        dm.add(int(c[0]), int(c[1]))
    dm.update()
    h = F.Loc2D(cov_blend=0.35)
    h.set_obstacles_world(obst)
    assert h.engine_origin().endswith("liblama_hip.so")
    x, y, yaw = M.SCAN_POSE
    for k, n in enumerate((180, 199, 290, 390, 1080)):
        pts = M.scan_of(n)
        assert len(pts) == n
        start = np.array([x, y + 0.05, yaw - 0.02 + 0.001 * k])
        o.set_pose(O.se2(*start))
        h.set_pose(*start)
        assert o.update(pts, O.se2(*start), float(k), force=True) == h.update(pts, start, float(k), force=True)
        assert np.abs(o.pose() - h.pose()).max() < 1e-7, n
        assert o.iterations() == h.iterations(), n
        assert abs(o.rmse() - h.rmse()) < 1e-9, n
        ol, hl = o.sampling_likelihoods(), h.sampling_likelihoods()
        assert len(hl) == 161 and np.allclose(ol, hl, rtol=1e-12, atol=1e-300), (n, np.abs(ol - hl).max())
        assert np.allclose(o.covar(), h.covar(), rtol=1e-6, atol=1e-12), n
    h.close()
