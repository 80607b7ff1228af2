"""CPU: what the feature render decides before any device call -- the shape checks of rasterizer.blend_features and of
render_gaussians' extra outputs, and the share_binning switch of CompositeRenderer."""
from types import SimpleNamespace

import pytest
import torch

from manus_amd._lib import ManusHipError


def test_blend_features_checks_its_request_before_any_device_call():
    from manus_amd.rasterizer import MAX_FEATURE_CHANNELS, blend_features
    assert MAX_FEATURE_CHANNELS == 32
    with pytest.raises(ManusHipError, match="33 channels"):
        blend_features(torch.zeros(10, 33))
    with pytest.raises(ManusHipError, match="0 channels"):
        blend_features(torch.zeros(10, 0), alpha=True)
    with pytest.raises(ManusHipError, match=r"\(N,C\)"):
        blend_features(torch.zeros(10))
    with pytest.raises(ManusHipError, match=r"\(N,C\)"):
        blend_features(torch.zeros(1, 2, 10, 3))
    with pytest.raises(ManusHipError, match=r"\(N,C\)"):
        blend_features([[0.0, 1.0]])
    with pytest.raises(ManusHipError, match="bg has 3 values for 4"):
        blend_features(torch.zeros(10, 4), bg=[0.0, 0.0, 0.0])
    with pytest.raises(ManusHipError, match="bg has 3 values for 0"):
        blend_features(bg=torch.zeros(3), depth=True)
    with pytest.raises(ManusHipError, match="nothing to render"):
        blend_features()


def test_render_gaussians_checks_the_extra_outputs_before_any_device_call():
    from manus_amd.render import render_gaussians
    cam = SimpleNamespace(fovx=1.0, fovy=1.0, height=8, width=8, world_view_transform=torch.eye(4),
                          full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))
    x = torch.zeros(4, 3)
    a = (x, torch.ones(4, 6), x, None, torch.ones(4, 1), cam, torch.ones(3), x)
    with pytest.raises(ManusHipError, match="40 channels"):
        render_gaussians(*a, extra_features=torch.zeros(4, 40))
    with pytest.raises(ManusHipError, match="one row per Gaussian"):
        render_gaussians(*a, extra_features=torch.zeros(5, 3))
    with pytest.raises(ManusHipError, match="one row per Gaussian"):
        render_gaussians(*a, extra_features=torch.zeros(1, 4, 3))
    with pytest.raises(ManusHipError, match="bg has 2 values for 3"):
        render_gaussians(*a, extra_features=torch.zeros(4, 3), feature_bg=[0.0, 1.0])
    with pytest.raises(ManusHipError, match="bg has 1 values for 0"):
        render_gaussians(*a, return_depth=True, feature_bg=[0.0])


def test_composite_renderer_stores_the_share_binning_switch():
    from manus_amd.modules import CompositeRenderer
    hand, obj = SimpleNamespace(), SimpleNamespace()
    assert CompositeRenderer(hand, obj).share_binning is False
    assert CompositeRenderer(hand, obj, share_binning=True).share_binning is True
    assert CompositeRenderer(hand, obj, "gt_eval", share_binning=1).share_binning is True


def test_contact_inputs_refuse_geometry_of_other_positions():
    from manus_amd.modules import Pred, contact_render_inputs
    h = Pred(posed_xyz=torch.zeros(3, 3), posed_cov=torch.zeros(3, 6), cano_xyz=torch.ones(3, 3))
    pred = Pred(h_out=h, o_out=Pred(posed_xyz=torch.zeros(2, 3)), cano_opacity=torch.ones(5, 1))
    skin = torch.rand(3, 3)
    first = contact_render_inputs(pred, None, "skin_wts", skin_colors=skin)
    again = contact_render_inputs(pred, None, "skin_wts", skin_colors=skin, geometry=first)
    assert again.posed_xyz is first.posed_xyz and again.posed_cov is first.posed_cov and again.opacity is first.opacity
    assert first.opacity is not contact_render_inputs(pred, None, "skin_wts", skin_colors=skin).opacity
    other = Pred(first, posed_xyz=h.cano_xyz)
    with pytest.raises(ValueError, match="other positions"):
        contact_render_inputs(pred, None, "skin_wts", skin_colors=skin, geometry=other)
