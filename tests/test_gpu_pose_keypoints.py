"""GPU tests of `pose_keypoints.KeypointChain`: every subset of {tracker, smoother, retargeter} over partitions of one clip
gives, bit for bit, the composition of the one-shot calls of the stages that are present.  Run with `-m gpu`.  The clip is
the two-person, 10-frame one of the tracker's tests, at 30 -> 16 frames/s: 10 source frames make 5 output frames, pushes of 1
make the retargeter return none, (3, 3, 4) crosses an output frame inside a push.  No kernel's geometry is at stake here:
the stages' own tests cover that."""
import itertools

import pytest
import torch

import self_forcing_amd as sfa
from test_gpu_pose_track import DEV, SIZE, swapping_pair

pytestmark = pytest.mark.gpu
KW = dict(beta=0.7, max_gap=2)
PARTITIONS = ((10,), (1,) * 10, (3, 3, 4), (1, 9))
SUBSETS = [s for r in range(4) for s in itertools.combinations(("tracker", "smoother", "retargeter"), r)]


@pytest.fixture(scope="module")
def clip():
    _, mixed, ref = swapping_pair(15, 10)
    return mixed, ref


def bits(t):
    return torch.as_tensor(t).cpu().contiguous().view(torch.int32)


def one_shot(subset, mixed, ref):
    """The composition of the one-shot calls of the stages in `subset`"""
    out = torch.from_numpy(mixed).to(DEV)
    if "tracker" in subset:
        out = sfa.PoseTracker(device=DEV).track(out).keypoints
    if "smoother" in subset:
        out = sfa.PoseSmoother(device=DEV).smooth(out, 30, **KW)
    if "retargeter" in subset:
        out = sfa.PoseRetargeter(device=DEV).retarget(out, ref, SIZE, source_fps=30)
    return out


def opened(subset, ref):
    stages = {}
    if "tracker" in subset:
        stages["tracker"] = sfa.PoseTracker(device=DEV).open_stream()
    if "smoother" in subset:
        stages["smoother"] = sfa.PoseSmoother(device=DEV).open_stream(30, **KW)
    if "retargeter" in subset:
        stages["retargeter"] = sfa.PoseRetargeter(device=DEV).open_stream(ref, SIZE, source_fps=30)
    return sfa.KeypointChain(**stages)


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_every_partition_equals_the_composition_of_the_one_shot_calls(clip, subset):
    mixed, ref = clip
    want = bits(one_shot(subset, mixed, ref))
    assert want.shape == (5 if "retargeter" in subset else 10, 2, 134, 3)
    if not subset:
        assert torch.equal(want, bits(mixed))                                            # no stage: the input's bits
    for parts in PARTITIONS:
        for pieces in (mixed, torch.from_numpy(mixed).to(DEV)):
            chain = opened(subset, ref)
            assert chain.in_pixels == ("retargeter" in subset) and len(chain.stages) == len(subset)
            got, at, planned = [], 0, []
            for n in parts:
                planned.append(chain.planned(n))
                got.append(chain.push(pieces[at:at + n]))
                at += n
            assert [len(g) for g in got] == planned and all(s.frames_in == 10 for s in chain.stages), (parts, planned)
            assert torch.equal(torch.cat([bits(g) for g in got]), want), (subset, parts, type(pieces))
            if "retargeter" in subset and len(parts) == 10:
                assert sorted(planned) == [0] * 5 + [1] * 5                              # every other push of one frame makes nothing final
