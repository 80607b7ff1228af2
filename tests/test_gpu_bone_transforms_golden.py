"""GPU: `mgr_bone_transforms` against recorded outputs, BIT FOR BIT.  tests/golden/bone_transforms.npz holds inputs (rest, posed
for B = 1 / 20 / 21 / 32) and what the kernel gave for them on an MI355X at the commit before its elimination and product moved
into csrc/bone_math.h (the parent's library and this one agreed on a sha256 over 241 k output floats; LAB.md).  The pose chain
(csrc/pose.hip) is held to the bits of this kernel by tests/test_gpu_pose_chain.py; this file holds the kernel itself in place, so
that a compiler that contracts the shared loops differently shows here and not as a silent drift of both."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bone_transforms.npz")


@pytest.mark.parametrize("B", [1, 20, 21, 32])
def test_bone_transforms_equals_the_recorded_bits(B):
    from manus_amd.transforms import bone_transforms
    d = np.load(GOLDEN)
    rest, posed, want = (torch.tensor(d["%s_%d" % (k, B)]).to("cuda:0") for k in ("rest", "posed", "T"))
    assert want.shape == (posed.shape[0], B + 1, 4, 4)
    for v in range(posed.shape[0]):
        assert torch.equal(bone_transforms(posed[v].contiguous(), rest, background=True), want[v]), v
        assert torch.equal(bone_transforms(posed[v].contiguous(), rest, background=False), want[v, :B]), v
