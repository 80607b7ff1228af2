"""CPU: the pose module (manus_amd/pose.py) and the ABI of the pose-gradient entries."""
import math
import os
import re

import torch

from oracle import torch_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_SYMBOLS = {"mgr_lbs_pose_bwd": 16, "mgr_lbs_pose_workspace_bytes": 3, "mgr_views_backward_pose": 39,
                "mgr_views_pose_workspace_bytes": 3}


def test_pose_correction_is_the_identity_at_zero():
    from manus_amd.pose import PoseCorrection
    g = torch.Generator().manual_seed(1)
    posed = torch.randn((20, 4, 4), generator=g)
    posed[:, 3, :] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    pc = PoseCorrection(3, 20)
    assert pc.rotvec.shape == pc.trans.shape == (3, 20, 3)
    assert float(pc.rotvec.detach().abs().max()) == 0.0 and float(pc.trans.detach().abs().max()) == 0.0
    for f in range(3):
        assert torch.equal(pc(posed, f), posed)
    out = pc(posed, 1)
    out.sum().backward()                                 # differentiable at zero: finite, non-trivial gradients
    assert torch.isfinite(pc.rotvec.grad).all() and float(pc.rotvec.grad[1].abs().max()) > 0.0
    assert float(pc.rotvec.grad[0].abs().max()) == 0.0


def test_pose_correction_rotation_is_orthonormal():
    from manus_amd.pose import PoseCorrection
    g = torch.Generator().manual_seed(2)
    pc = PoseCorrection(4, 20)
    with torch.no_grad():
        d = torch.randn((4, 20, 3), generator=g)
        pc.rotvec.copy_(d / d.norm(dim=-1, keepdim=True) * torch.rand((4, 20, 1), generator=g) * (math.pi / 2))
        pc.rotvec[0, 0] = torch.tensor([math.pi / 2, 0.0, 0.0])
        pc.rotvec[0, 1] = torch.tensor([1e-4, -2e-4, 1e-5])          # the series branch
        pc.trans.copy_(torch.randn((4, 20, 3), generator=g))
    eye = torch.eye(4).repeat(20, 1, 1)
    for f in range(4):
        C = pc(eye, f)
        R = C[:, :3, :3]
        assert float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 8 * 2.0 ** -23
        assert float((torch.linalg.det(R) - 1.0).abs().max()) < 8 * 2.0 ** -23
        assert torch.equal(C[:, :3, 3], pc.trans[f]) and torch.equal(C[:, 3, :], eye[:, 3, :])
    ang = torch.acos(((pc(eye, 0)[0, :3, :3]).diagonal().sum() - 1) / 2)
    assert abs(float(ang) - math.pi / 2) < 1e-6


def test_pose_backward_equals_autograd_through_bone_transforms():
    from manus_amd.pose import pose_backward
    g = torch.Generator().manual_seed(3)
    for lead, background in (((), True), ((3,), True), ((), False)):
        B = 20
        rest = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1) + 0.3 * torch.randn((B, 4, 4), generator=g, dtype=torch.float64)
        posed = torch.randn(lead + (B, 4, 4), generator=g, dtype=torch.float64).requires_grad_(True)
        dT = torch.randn(lead + (B + (1 if background else 0), 4, 4), generator=g, dtype=torch.float64)
        flat = posed.reshape((-1, B, 4, 4))
        T = torch.stack([tr.bone_transforms(flat[k], rest, background=background) for k in range(flat.shape[0])]).reshape(dT.shape)
        (T * dT).sum().backward()
        got = pose_backward(dT, posed.detach(), rest, background=background)
        assert got.shape == posed.shape
        assert float((got - posed.grad).abs().max()) <= 1e-12 * max(1.0, float(posed.grad.abs().max()))


def test_pose_symbols_are_declared_and_bound_with_matching_arity():
    from manus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "manus_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, arity in POSE_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "not declared in include/manus_hip.h: " + name
        assert len(m.group(1).split(",")) == arity, (name, len(m.group(1).split(",")))
        assert name in _lib.SIGNATURES, "python binding missing for " + name
        assert len(_lib.SIGNATURES[name][1]) == arity, (name, len(_lib.SIGNATURES[name][1]))
    assert _lib.SIGNATURES["mgr_views_backward_pose"][1][:35] == _lib.SIGNATURES["mgr_views_backward"][1][:35]
    assert hasattr(_lib.lib(), "mgr_views_backward_pose") and hasattr(_lib.lib(), "mgr_lbs_pose_bwd")
    # argument validation needs no GPU
    L = _lib.lib()
    assert L.mgr_lbs_pose_workspace_bytes(3, 777, 21) == 4 * 3 * 21 * 12 * 4
    assert L.mgr_lbs_pose_workspace_bytes(1, 10 ** 6, 21) == 1024 * 21 * 12 * 4
    assert L.mgr_views_pose_workspace_bytes(8, 300000, 21) == 1024 * 8 * 21 * 12 * 4 + 300000 * 8     # partial slots | slot flags
    assert L.mgr_lbs_pose_bwd(1, 5, 21, None, None, None, None, None, None, None, None, 12, None, None, 0, None) != 0
    assert b"skin_w" in L.mgr_last_error()
