"""GPU: coarse-to-fine and Huber-weighted tracking (TsdfVolume.track_pyramid, StereoRig.track(..., levels=, huber=)) against
the fp64 oracle loops of tests/test_pyramid_host.py, whose text says how the scene and the offset were decided on the CPU.
No offset of that scene separates the single-level loop from the three-level one, so the condition here is the one that holds on the
oracle: at POSE1 the three-level loop ends within 2 x the fp64 pyramid oracle's error in both components (the margin of
test_tracking_the_corner_scene) and no farther from the truth than the GPU's single-level loop, up to SLACK of that
loop's error (below)."""
import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import tracking
from tests.test_gpu_tsdf import put
from tests.test_icp_host import CORNER, POSE0, TRACK, corner_disparity, pose_error
from tests.test_pyramid_host import (HUBER, LEVELS, MAX_DISTANCE, PYRAMID_OFFSET, SIZE, huber_frame, huber_tracked, offset_pose,
                                     scanned, scene_matrix)
from tests.test_register_depth_host import simple_rig
from tests.test_tsdf_host import general_pose

pytestmark = pytest.mark.gpu

NAN = float('nan')
# How much farther from the truth than the single-level loop the three-level loop may end, as a share of the single-level
# loop's error.  Both loops end with level-0 iterations on the same frame and the same model and stop when a step is below
# tolerance = 1e-6, which is under 0.1 % of the converged error (2.5e-3 rad, 1.4e-3 m on the oracle); the float32 rows
# carry REL32 = 2.4e-7 of metre-sized terms, less again.  What is left is association: the two loops reach level 0 from
# different transforms, a pixel whose projection lies within float32 rounding of a pixel boundary may pair with either
# neighbour at the end, and the oracle holds such undecided rows under 2 % of the rows at every iteration.  A share s of
# rows decided otherwise moves the least-squares solution by at most about s of the residual field, which at convergence
# is the remaining error itself: 2 %.
SLACK = 0.02


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def volume(dev):
    v = pds.TsdfVolume(CORNER['origin'], CORNER['voxel_size'], CORNER['dims'], CORNER['truncation'], device=dev)
    return v.integrate(put(dev, corner_disparity(POSE0, SIZE)[None]), scene_matrix(), pose=POSE0)


def same(a, b):
    return (a.pose.tobytes() == b.pose.tobytes() and a.rmse.tobytes() == b.rmse.tobytes() and
            a.inliers.tolist() == b.inliers.tolist() and a.status.tolist() == b.status.tolist() and a.iterations == b.iterations)


def test_one_level_is_the_default_call(dev, volume):
    frame = put(dev, corner_disparity(offset_pose(PYRAMID_OFFSET), SIZE)[None])
    default = volume.track(frame, scene_matrix(), POSE0, **TRACK)
    explicit = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=1, huber=None, max_difference=None, **TRACK)
    assert default.status.tolist() == [tracking.TRACKED] and same(default, explicit)
    listed = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=1, **dict(TRACK, iterations=[TRACK['iterations']]))
    assert same(default, listed)


def test_three_levels_at_the_chosen_offset(dev, volume):
    truth = offset_pose(PYRAMID_OFFSET)
    frame = put(dev, corner_disparity(truth, SIZE)[None])
    t = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=LEVELS, **TRACK)
    single = volume.track(frame, scene_matrix(), POSE0, **TRACK)
    oracle_pose, history, status = scanned(PYRAMID_OFFSET, LEVELS)
    assert status == tracking.TRACKED and t.status.tolist() == [tracking.TRACKED]
    start, want = pose_error(POSE0, truth), pose_error(oracle_pose, truth)
    got, got1 = pose_error(t.pose[0], truth), pose_error(single.pose[0], truth)
    print('start %.3e rad %.3e m; the fp64 pyramid oracle %.3e rad %.3e m (%d systems); the GPU, %d levels: %.3e rad %.3e m, '
          '%d systems, rmse %.3e, %d inliers; the GPU, one level: %.3e rad %.3e m, %d systems' %
          (start + want + (len(history), LEVELS) + got + (t.iterations, t.rmse[0], t.inliers[0]) + got1 + (single.iterations,)))
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1]
    print('three levels against one: %+.3e rad (%+.3f %%), %+.3e m (%+.3f %%)' %
          (got[0] - got1[0], 100 * (got[0] - got1[0]) / got1[0], got[1] - got1[1], 100 * (got[1] - got1[1]) / got1[1]))
    assert got[0] <= (1 + SLACK) * got1[0] and got[1] <= (1 + SLACK) * got1[1]
    assert LEVELS <= t.iterations <= LEVELS * TRACK['iterations'] and t.inliers[0] >= 0.2 * SIZE[0] * SIZE[1]
    R = t.pose[0, :, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    # iterations and max_distance per level, indexed by level
    listed = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=LEVELS, max_distance=[MAX_DISTANCE] * LEVELS,
                                  **dict(TRACK, iterations=[TRACK['iterations']] * LEVELS))
    assert same(listed, t)
    short = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=LEVELS, **dict(TRACK, iterations=(1, 2, 3), tolerance=0.0))
    assert short.iterations == 6 and short.status.tolist() == [tracking.TRACKED]


def test_a_blind_entry_beside_a_tracked_one(dev, volume):
    frame = put(dev, corner_disparity(offset_pose(PYRAMID_OFFSET), SIZE)[None])
    frames = torch.cat([frame, torch.full_like(frame, NAN)])
    mixed = volume.track_pyramid(frames, scene_matrix(), np.stack([POSE0, POSE0]), levels=LEVELS, **TRACK)
    assert mixed.status.tolist() == [tracking.TRACKED, tracking.TOO_FEW_ROWS] and (mixed.pose[1] == POSE0).all()
    assert mixed.inliers[1] == 0 and np.isnan(mixed.rmse[1])
    alone = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=LEVELS, **TRACK)
    assert pose_error(mixed.pose[0], alone.pose[0])[1] <= 1e-9 and pose_error(mixed.pose[0], alone.pose[0])[0] <= 1e-9


def test_huber_on_the_blob_frame(dev, volume):
    d, truth = huber_frame()
    frame = put(dev, d[None])
    oracle_pose, _, status = huber_tracked(HUBER['huber'])
    assert status == tracking.TRACKED
    t = volume.track_pyramid(frame, scene_matrix(), POSE0, levels=1, huber=HUBER['huber'], **TRACK)
    plain = volume.track(frame, scene_matrix(), POSE0, **TRACK)
    want, got, unweighted = pose_error(oracle_pose, truth), pose_error(t.pose[0], truth), pose_error(plain.pose[0], truth)
    print('the blob frame: the fp64 Huber oracle %.3e rad %.3e m; the GPU with huber %.3e rad %.3e m, without %.3e rad %.3e m' %
          (want + got + unweighted))
    assert t.status.tolist() == [tracking.TRACKED]
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1]


def test_through_the_rig(dev):
    rig = simple_rig(256, 128)
    yy, xx = np.mgrid[0:128, 0:256].astype(np.float64)
    d = 20.0 + 0.02 * xx - 0.01 * yy
    d[40:90, 100:180] = 26.0
    d = put(dev, d.astype(np.float32)[None])
    near = float(rig.reproject(d, depth_only=True).median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    pose = general_pose(1)
    vol = rig.integrate(rig.tsdf_volume(device=dev, **geometry), d, pose)
    through = rig.track(vol, d, pose, iterations=3, levels=3, huber=near / 64)
    camera = (rig.P1[0, 0], rig.P1[1, 1], rig.P1[0, 2], rig.P1[1, 2], 0.0)
    explicit = vol.track_pyramid(d, rig.reprojection_matrix('rectified'), pose, camera=camera, size=(256, 128),
                                 iterations=3, levels=3, huber=near / 64)
    # without the three keywords the rig goes to track, as before
    assert same(rig.track(vol, d, pose, iterations=3), vol.track(d, rig.reprojection_matrix('rectified'), pose, camera=camera,
                                                                 size=(256, 128), iterations=3))
    assert isinstance(through, pds.Tracking) and through.inliers[0] > 1000 and through.iterations >= 3
    assert same(through, explicit)
