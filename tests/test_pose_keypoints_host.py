"""Host tests of `pose_keypoints.KeypointChain`, the seam between the keypoint stages and their callers, with no device: the
rule between a tracker and a smoother, the order the stages run in (read from whose error comes first), and the plan."""
import numpy as np
import pytest

import self_forcing_amd as sfa
from self_forcing_amd import pose_retarget_reference as rr

F32 = np.float32
K = np.zeros((5, 1, 134, 3), F32)


def streams(max_gap=0, max_age=2):
    """A tracker's, a smoother's and a retargeter's stream (30 -> 16 frames/s), none of which has a device to run on"""
    return (sfa.PoseTracker(device="cpu").open_stream(max_age=max_age), sfa.PoseSmoother(device="cpu").open_stream(30, max_gap=max_gap),
            sfa.PoseRetargeter(device="cpu").open_stream(K[0], (24, 40), source_fps=30))


def test_the_chain_is_exported():
    assert sfa.KeypointChain is sfa.pose_keypoints.KeypointChain and {"KeypointChain", "pose_keypoints"} <= set(sfa.__all__)
    assert sfa.pose_render.as_tensor is sfa.pose_keypoints.as_tensor


@pytest.mark.parametrize("max_gap,max_age", [(3, 2), (1, 0), (65535, 65534)])
def test_a_smoother_that_bridges_more_than_the_tracker_waits_is_refused(max_gap, max_age):
    tracker, smoother, retargeter = streams(max_gap, max_age)
    for more in ({}, {"retargeter": retargeter}):
        with pytest.raises(ValueError, match="one person towards another") as e:
            sfa.KeypointChain(tracker=tracker, smoother=smoother, **more)
        assert f"max_gap = {max_gap}" in str(e.value) and f"max_age + 1 = {max_age + 1}" in str(e.value)
    assert sfa.KeypointChain.bridges_two_people(max_gap, max_age)
    sfa.KeypointChain(smoother=smoother, retargeter=retargeter)                          # the rule is between those two stages alone
    sfa.KeypointChain(tracker=tracker, retargeter=retargeter)


def test_max_gap_equal_to_max_age_is_within_the_guarantee():
    tracker, smoother, _ = streams(3, 3)
    assert sfa.KeypointChain(tracker, smoother).stages == [tracker, smoother] and not sfa.KeypointChain.bridges_two_people(3, 3)


def test_the_tracker_runs_first_and_the_smoother_second():
    tracker, smoother, retargeter = streams()
    with pytest.raises(ValueError, match="PoseTracker: expected a CUDA/ROCm device"):
        sfa.KeypointChain(tracker, smoother, retargeter).push(K)
    with pytest.raises(ValueError, match="PoseSmoother: expected a CUDA/ROCm device"):
        sfa.KeypointChain(smoother=smoother, retargeter=retargeter).push(K)
    with pytest.raises(ValueError, match="PoseRetargeter: expected a CUDA/ROCm device"):
        sfa.KeypointChain(retargeter=retargeter).push(K)
    assert (tracker.frames_in, smoother.frames_in, retargeter.frames_in) == (0, 0, 0)    # a failed push leaves every stage as it was
    assert tracker.state is None and smoother.state is None and retargeter.frames_out == 0


@pytest.mark.parametrize("frames_in", [0, 1, 7])
def test_the_plan_is_the_retargeters(frames_in):
    _, smoother, retargeter = streams()
    chain = sfa.KeypointChain(smoother=smoother, retargeter=retargeter)
    assert chain.in_pixels
    retargeter.frames_in = frames_in                                                     # a stream that has taken that many source frames
    assert (retargeter.params.num, retargeter.params.den) == (15, 8)
    for n in range(1, 13):
        assert chain.planned(n) == rr.plan(frames_in, n, 15, 8)[1], n
    assert sum(chain.planned(n) != n for n in range(1, 13)) >= 10                        # 30 -> 16 frames/s: the plan is not the identity


def test_without_a_retargeter_every_source_frame_is_an_output_frame():
    tracker, smoother, _ = streams()
    for chain in (sfa.KeypointChain(), sfa.KeypointChain(tracker), sfa.KeypointChain(tracker, smoother)):
        assert not chain.in_pixels and [chain.planned(n) for n in range(1, 13)] == list(range(1, 13))
    assert sfa.KeypointChain().push(K) is K                                              # no stage: the batch as it came
