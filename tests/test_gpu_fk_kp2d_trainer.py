"""GPU: `engine.Trainer(pose=...)` with a `pose.KinematicPoseRefiner` that carries the 2-D keypoint term beside f23's terms, against
hand-written loops, bit for bit -- leaves, theta, moments, losses, `last_terms` and `loss_pose_prior`.

Set-up and loops of tests/test_gpu_fk_terms_trainer.py (3 frames x 4 cameras at 64x48, 2000 Gaussians, 3 views per step, refiner
from step 2 on every second step), with that module's `refiner` replaced by one that also sets detections: the store's 3-D
keypoints seen by four cameras around them (`fk_kp2d_ref.look_at`), 3 pixels of noise, confidences in [0.5, 1], one detection
missing (weight 0, NaN target)."""
import pytest
import torch

import fk_kp2d_ref as Q
import test_gpu_fk_terms_trainer as TT
from test_gpu_fk_trainer import capture, same  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TERMS2D = dict(TT.TERMS, w_kp2d=0.002, kp2d_delta=4.0)
ONLY2D = dict(w_kp2d=0.002, kp2d_delta=4.0)
ORIGINAL = TT.refiner


def detections(store, ds):
    from manus_amd.pose import keypoints_of_store, project_keypoints, projection_matrices
    p = keypoints_of_store(store, ds.index_list).cpu().double()                            # (F,21,3)
    g = torch.Generator().manual_seed(606)
    centre = p.reshape(-1, 3).mean(0)
    radius = float((p.reshape(-1, 3) - centre).norm(dim=1).max())
    ext = torch.stack([Q.look_at(centre + 4.0 * radius * d, -d) for d in Q.sphere(4, g)])
    Kin = torch.tensor([[Q.FOCAL, 0.0, Q.CENTRE[0]], [0.0, Q.FOCAL, Q.CENTRE[1]], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(4, 1, 1)
    proj = projection_matrices(Kin, ext)
    t = project_keypoints(proj, p) + 3.0 * torch.randn((p.shape[0], 4, 21, 2), generator=g, dtype=torch.float64)
    s = 0.5 + 0.5 * torch.rand((p.shape[0], 4, 21), generator=g, dtype=torch.float64)
    s[1, 2, 5] = 0.0
    t[1, 2, 5] = float("nan")
    return proj, t, s


def with_detections(default_terms):
    """`test_gpu_fk_terms_trainer.refiner` plus `set_keypoints_2d`; the module's default TERMS stand for `default_terms`."""
    def refiner(ds, store, hc, terms=TT.TERMS, keypoints=True):
        from manus_amd.pose import keypoint_offsets
        ref = ORIGINAL(ds, store, hc, default_terms if terms is TT.TERMS else terms, keypoints)
        rest = ds[0]["bones_rest"]
        b, o = (None, None) if keypoints else keypoint_offsets(rest.transforms, rest.heads, rest.tails)
        ref.set_keypoints_2d(*detections(store, ds), bones=b, offsets=o)
        return ref
    return refiner


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("terms", ["all", "only2d"])
def test_trainer_equals_the_hand_written_loop(capture, fused, terms, monkeypatch):  # noqa: F811
    monkeypatch.setattr(TT, "refiner", with_detections(TERMS2D if terms == "all" else ONLY2D))
    keypoints = terms == "all"
    a, _, tr = TT.trainer_run(capture, fused, keypoints=keypoints)
    TT.compare_all(a, TT.hand_loop(capture, fused, keypoints=keypoints), "kp2d %s, fused=%s" % (terms, fused))
    assert [r["steps"] for r in a] == [0, 0, 1, 1, 2, 2] and TT.priors_at(a) == [2, 4]
    t, p, e2d = tr.pose.last_terms, tr.pose.last_prior, tr.pose.last_kp2d
    assert torch.equal(t, a[4]["terms"]) and t.shape == (4,) and p.data_ptr() == t[3:].data_ptr() and e2d.data_ptr() == p.data_ptr() + 8
    assert float(e2d) > 0.0 and float(p) == ((float(t[0]) + float(t[1])) + float(t[2])) + float(e2d)
    if terms == "only2d":
        assert bool((t[:3] == 0.0).all())
    # the term moves the angles: another run than the same refiner without it
    monkeypatch.setattr(TT, "refiner", ORIGINAL)
    plain = TT.trainer_run(capture, fused, terms=TT.TERMS if keypoints else None, keypoints=keypoints)[0]
    assert not torch.equal(plain[2]["state"]["theta"], a[2]["state"]["theta"])
    same(plain[1]["state"], a[1]["state"], "before the first step of the angles")


@pytest.mark.parametrize("fused", [True, False])
def test_zero_weight_with_detections_set_equals_a_refiner_without_either(capture, fused, monkeypatch):  # noqa: F811
    monkeypatch.setattr(TT, "refiner", with_detections(dict(TT.TERMS, w_kp2d=0.0, kp2d_delta=4.0)))
    zero, _, tr = TT.trainer_run(capture, fused)
    assert tr.pose.kp2d is not None and tr.pose.last_kp2d is None
    monkeypatch.setattr(TT, "refiner", ORIGINAL)
    TT.compare_all(zero, TT.trainer_run(capture, fused)[0], "w_kp2d = 0 with detections, fused=%s" % fused)
    # and with no term at all: the plain entry
    monkeypatch.setattr(TT, "refiner", with_detections(None))
    bare = TT.trainer_run(capture, fused, terms=None, keypoints=False)[0]
    monkeypatch.setattr(TT, "refiner", ORIGINAL)
    TT.compare_all(bare, TT.trainer_run(capture, fused, terms=None, keypoints=False)[0], "no term, fused=%s" % fused)
    assert TT.priors_at(bare) == []


def test_state_through_a_checkpoint_resumes_bit_for_bit(capture, tmp_path, monkeypatch):  # noqa: F811
    """f23's checkpoint test on the refiner with the 2-D term on: weights and detections are configuration, the state is theta, m,
    v and steps."""
    monkeypatch.setattr(TT, "refiner", with_detections(TERMS2D))
    TT.test_state_through_a_checkpoint_resumes_bit_for_bit(capture, tmp_path)
