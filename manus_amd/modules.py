"""Forward passes of the MANUS training modules on the HIP kernels.

Mirrors (brown-ivl/manus):
  hand_forward      src/modules/hand_dynamic.py:86-137   TrainingModule.forward
  object_forward    src/modules/object.py:32-41
  composite_forward src/modules/composite.py:50-78
  composite_pred    the same with the reference's `h_out` / `o_out` carried along
  render_contacts   src/modules/composite.py:143-214   Composite.render_contacts (all eight render types)
  CompositeRenderer src/modules/composite.py:83-125    Composite.render ('gt_eval', 'acc_gt_eval', 'results', 'nocs')
Each takes the reference's model object (anything exposing `_xyz`, `_scaling`,
`_rotation`, `get_features`, `get_opacity`, and for the hand `grid_center`,
`grid_scale`, `grid_weights`) and the reference's batch dict, and returns the same
dict of tensors the reference returns (attribute-accessible).
"""
import torch

from .ops import lbs_cov, skin_weights
from .transforms import bone_transforms


class Pred(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def device_grid(model):
    """The reference re-uploads the (D,H,W,21) grid on every call
    (gaussian_utils.py:169); here it is uploaded once and cached on the model."""
    from .ops import SkinGrid
    g = getattr(model, "_mgr_grid_dev", None)
    dev = model._xyz.device
    if g is None or g.data.device != dev:
        g = SkinGrid(model.grid_weights, dev)
        model._mgr_grid_dev = g
    return g


def hand_forward(model, batch, background_transform=True, full_tf=True):
    cano_xyz = model._xyz
    dev = cano_xyz.device
    posed_t = torch.as_tensor(batch["bones_posed"].transforms, dtype=torch.float32).to(dev)
    rest_t = torch.as_tensor(batch["bones_rest"].transforms, dtype=torch.float32).to(dev)
    T = bone_transforms(posed_t, rest_t, background=background_transform)
    w = skin_weights(cano_xyz, device_grid(model),
                     torch.as_tensor(model.grid_center).to(dev), torch.as_tensor(model.grid_scale).to(dev))
    assert w.shape[-1] == T.shape[0]  # hand_dynamic.py:104
    # full_tf: the reference's (N,4,4) -- written in that layout by the LBS kernel and read in place by the SH operator
    # (render.calculate_colors_from_sh): no cat of the constant row, no slice copy, nothing in between in the backward either
    pxyz, pcov, tf = lbs_cov(cano_xyz, model._scaling, model._rotation, w, T, tf44=full_tf)
    return Pred(posed_xyz=pxyz[0], posed_cov=pcov[0], cano_xyz=cano_xyz, cano_features=model.get_features,
                cano_opacity=model.get_opacity, tf=tf[0], skin_wts=w)


def object_forward(model, batch=None):
    pxyz, pcov, _ = lbs_cov(model._xyz, model._scaling, model._rotation, None, None)
    return Pred(posed_xyz=model._xyz, posed_cov=pcov[0], cano_xyz=model._xyz,
                cano_features=model.get_features, cano_opacity=model.get_opacity)


def _composite(h, o):
    n_o = o.posed_xyz.shape[0]
    eye = torch.eye(4, dtype=torch.float32, device=h.tf.device)[None].expand(n_o, 4, 4)
    return Pred(posed_xyz=torch.cat([h.posed_xyz, o.posed_xyz]), posed_cov=torch.cat([h.posed_cov, o.posed_cov]),
                cano_xyz=torch.cat([h.cano_xyz, o.cano_xyz]),
                cano_features=torch.cat([h.cano_features, o.cano_features]),
                cano_opacity=torch.cat([h.cano_opacity, o.cano_opacity]), tf=torch.cat([h.tf, eye]),
                n_hand=h.posed_xyz.shape[0])


def composite_forward(hand_model, obj_model, batch):
    """Concatenate hand (skinned) and object (identity tf) Gaussians, composite.py:50-78."""
    return _composite(hand_forward(hand_model, batch), object_forward(obj_model, batch))


def composite_pred(hand_model, obj_model, batch):
    """`composite_forward` that also carries the two bodies' own outputs as `h_out` / `o_out` (the reference's `pred.h_out`,
    `pred.o_out`, composite.py:67-77; `o_out.tf` is None as in src/modules/object.py:32-41), which the contact renders read."""
    h = hand_forward(hand_model, batch)
    o = object_forward(obj_model, batch)
    pred = _composite(h, o)
    pred["h_out"], pred["o_out"] = h, Pred(o, tf=None)
    return pred


RENDER_TYPES = ("object_only", "hand_only", "nocs_hand_only", "nocs_object_only", "accumulated", "acc_gt_eval", "skin_wts")


def _canonical_cov(model):
    """`model.get_covariance()` of src/models/gaussian.py:84-93 (the unposed covariances, (N,6)); a model that does not have
    the method gets them from the LBS kernel with the identity transform, like `object_forward`."""
    fn = getattr(model, "get_covariance", None)
    if fn is not None:
        return fn()
    return lbs_cov(model._xyz, model._scaling, model._rotation, None, None)[1][0]


def _contact(pt1, pt2, search, c_thresh):
    """(value, int32 index of the nearest point) of pt1 against pt2."""
    from . import contact
    if search == "near":
        value, idx, _ = contact.contact_near(pt1, pt2, c_thresh)
        return value, idx
    if search == "brute":
        dist, idx = contact._nearest(pt1, pt2, True)
        return contact.contact_values(dist, c_thresh), idx
    raise ValueError("search is 'near' or 'brute', got %r" % (search,))


def contact_render_inputs(pred, camera, render_type, cmap_type="magma", alpha=0.3, acc_dist=None, hand_model=None,
                          obj_model=None, nocs_grid=None, skin_colors=None, search="near", c_thresh=0.004,
                          reference_opacity_rows=False, geometry=None):
    """What `render_contacts` hands to `render_gaussians` for one render type: Pred(dist, posed_xyz, posed_cov,
    colors_precomp, opacity), with the reference's choice of positions / covariances / colours (composite.py:150-206).

    `geometry`: what this function returned for another render type of the SAME positions ('hand_only' / 'accumulated',
    'acc_gt_eval' / 'skin_wts'): covariances and opacities are then taken from it -- the same tensor objects, nothing computed
    again -- and only the colours are this type's (CompositeRenderer(share_binning=True)).

    Opacities: the reference passes the opacities of the WHOLE composite (hand rows first) next to the n rows of ONE body,
    and its rasterizer reads the first n of them -- right for the hand, the hand's first n_object values for the object.
    Here every body gets its own rows; `reference_opacity_rows=True` takes `cano_opacity[:n]` like the reference."""
    from . import contact
    from .render import calculate_colors_from_sh
    h, o = pred.h_out, pred.o_out
    n_h = h.posed_xyz.shape[0]
    dist = None
    body = "hand"

    def sh_colors_of(p):
        return calculate_colors_from_sh(p.cano_xyz, p.cano_features, p.cano_xyz, camera, 3, p.get("tf"))

    def need(x, name):
        if x is None:
            raise ValueError("render type %r needs %s" % (render_type, name))
        return x

    if render_type == "object_only":
        body = "object"
        dist, _ = _contact(o.posed_xyz, h.posed_xyz, search, c_thresh)
        xyz, cov = o.posed_xyz, _canonical_cov(need(obj_model, "obj_model"))
        colors = contact.contact_colors(dist, cmap_type, sh_colors_of(o), alpha)
    elif render_type == "hand_only":
        dist, _ = _contact(h.posed_xyz, o.posed_xyz, search, c_thresh)
        xyz, cov = h.cano_xyz, _canonical_cov(need(hand_model, "hand_model"))
        colors = contact.contact_colors(dist, cmap_type, sh_colors_of(h), alpha)
    elif render_type == "nocs_hand_only":
        dist, _ = _contact(h.posed_xyz, o.posed_xyz, search, c_thresh)
        xyz, cov = h.cano_xyz, _canonical_cov(need(hand_model, "hand_model"))
        colors = contact.contact_table_colors(dist, need(nocs_grid, "nocs_grid"))
    elif render_type == "nocs_object_only":
        body = "object"
        dist, idx = _contact(o.posed_xyz, h.posed_xyz, search, c_thresh)
        xyz, cov = o.posed_xyz, _canonical_cov(need(obj_model, "obj_model"))
        colors = contact.contact_table_colors(dist, need(nocs_grid, "nocs_grid"), idx)
    elif render_type == "accumulated":
        dist = need(acc_dist, "acc_dist")
        # (the one type whose covariances would be computed again for a shared render: taken from `geometry` when given)
        xyz, cov = h.cano_xyz, geometry.posed_cov if geometry is not None else _canonical_cov(need(hand_model, "hand_model"))
        colors = contact.contact_colors(dist, cmap_type, sh_colors_of(h), alpha)
    elif render_type == "acc_gt_eval":
        dist = need(acc_dist, "acc_dist")
        xyz, cov = h.posed_xyz, h.posed_cov
        colors = contact.contact_colors(dist, cmap_type)
    elif render_type == "skin_wts":
        xyz, cov = h.posed_xyz, h.posed_cov
        colors = need(skin_colors, "skin_colors").to(xyz.device)
    else:
        raise ValueError("unknown render_type %r (one of %s)" % (render_type, ", ".join(RENDER_TYPES)))
    n = xyz.shape[0]
    if reference_opacity_rows or body == "hand":
        opacity = pred.cano_opacity[:n]
    else:
        opacity = pred.cano_opacity[n_h:]
    if geometry is not None:
        if geometry.posed_xyz is not xyz:
            raise ValueError("geometry= comes from a render type with other positions than %r" % (render_type,))
        cov, opacity = geometry.posed_cov, geometry.opacity
    return Pred(dist=dist, posed_xyz=xyz, posed_cov=cov, colors_precomp=colors, opacity=opacity)


def render_contacts(pred, batch, camera, render_type="hand_only", cmap_type="magma", alpha=0.3, acc_dist=None, hand_model=None,
                    obj_model=None, nocs_grid=None, skin_colors=None, search="near", c_thresh=0.004,
                    reference_opacity_rows=False):
    """Composite.render_contacts, composite.py:143-214: (dist, image (H,W,3)).  `pred` comes from `composite_pred`; `dist` is
    the contact value in [0,1] the render was coloured by (None for 'skin_wts').  The search is on the grid (`search="near"`,
    `mgr_contact_near`) unless `search="brute"`; the colour map is looked up on the device."""
    from .render import render_gaussians
    r = contact_render_inputs(pred, camera, render_type, cmap_type, alpha, acc_dist, hand_model, obj_model, nocs_grid,
                              skin_colors, search, c_thresh, reference_opacity_rows)
    img = render_gaussians(r.posed_xyz, r.posed_cov, pred.cano_xyz, pred.cano_features, r.opacity, camera, batch["bg_color"],
                           r.colors_precomp, sh_degree=3, tf=pred.tf)["render"]
    return r.dist, img


class CompositeRenderer:
    """Composite.render of composite.py:83-125 for a grasp sequence: `render(batch)` returns the composite Pred with
    `render` = the panels of the frame side by side, (H, k*W, 3).

    The reference appends every frame's hand contact values to a list and sums `torch.stack(list)` again on every frame;
    here the running sum lives on the device and frame t adds its values to it (`acc += h_dist`, in frame order: fp32
    additions ((h0 + h1) + h2) + ...).  `reset()` starts a new sequence."""

    def __init__(self, hand_model, obj_model, render_contact_type="results", nocs_grid=None, skin_colors=None, acc_contacts=None,
                 sh_degree=3, search="near", c_thresh=0.004, reference_opacity_rows=False, share_binning=False):
        self.hand_model, self.obj_model = hand_model, obj_model
        # share_binning: the second render of a pair that shows the same Gaussians through the same camera in other colours
        # ('hand_only' + 'accumulated', 'acc_gt_eval' + 'skin_wts') is composited on the first render's tile lists
        # (rasterizer.blend_features) instead of projecting, sorting and binning them again -- the same contributions, the
        # panel equal up to the rounding of its sums
        self.share_binning = bool(share_binning)
        self.render_contact_type = render_contact_type
        self.nocs_grid, self.skin_colors, self.acc_contacts = nocs_grid, skin_colors, acc_contacts
        self.sh_degree = sh_degree
        self.kw = dict(hand_model=hand_model, obj_model=obj_model, nocs_grid=nocs_grid, skin_colors=skin_colors, search=search,
                       c_thresh=c_thresh, reference_opacity_rows=reference_opacity_rows)
        self.reset()

    def reset(self):
        self.acc = None
        self.n_frames = 0

    def _accumulate(self, h_dist):
        if self.acc is None:
            self.acc = h_dist.clone()
        else:
            self.acc.add_(h_dist)
        self.n_frames += 1
        return self.acc

    def save_accumulated(self, path):
        """The running sum of a 'gt_eval' / 'results' pass as the reference's `acc_contacts.npy` (on_test_epoch_end,
        composite.py:262-266): the hand from the first pass of scripts/train/eval.sh to the second."""
        import numpy as np
        if self.acc is None:
            raise ValueError("save_accumulated: no frame has been rendered with 'gt_eval' or 'results' yet")
        with open(path, "wb") as f:      # (np.save on a name would append '.npy' to one without it)
            np.save(f, self.acc.detach().cpu().numpy())

    def load_accumulated(self, path):
        """`acc_contacts` for 'acc_gt_eval' from such a file (on_test_epoch_start, composite.py:224-226), on the hand model's
        device."""
        import numpy as np
        self.acc_contacts = torch.from_numpy(np.load(path)).to(self.hand_model._xyz.device)
        return self.acc_contacts

    def _rgb(self, pred, batch):
        from .render import render_gaussians
        return render_gaussians(pred.posed_xyz, pred.posed_cov, pred.cano_xyz, pred.cano_features, pred.cano_opacity,
                                batch["camera"], batch["bg_color"], None, sh_degree=self.sh_degree, tf=pred.tf)

    def _first_of_pair(self, pred, batch, camera, rtype, *a, **k):
        """`render_contacts` that keeps what the second render of the pair shares: (inputs, image)."""
        from .rasterizer import context
        from .render import render_gaussians
        r = contact_render_inputs(pred, camera, rtype, *a, **dict(self.kw, **k))
        img = render_gaussians(r.posed_xyz, r.posed_cov, pred.cano_xyz, pred.cano_features, r.opacity, camera, batch["bg_color"],
                               r.colors_precomp, sh_degree=3, tf=pred.tf)["render"]
        r["camera"], r["workspace"] = camera, context(r.posed_xyz.device).last_ws
        return r, img

    def _second_of_pair(self, pred, batch, camera, first, rtype, *a, **k):
        """(dist, image) of `rtype` composited on the tile lists of the render `first` came from."""
        from .rasterizer import blend_features, context
        r = contact_render_inputs(pred, camera, rtype, *a, **dict(self.kw, geometry=first, **k))
        assert r.posed_xyz is first.posed_xyz and r.posed_cov is first.posed_cov and r.opacity is first.opacity
        assert camera is first.camera and context(r.posed_xyz.device).last_ws is first.workspace
        out = blend_features(r.colors_precomp, bg=batch["bg_color"], device=r.posed_xyz.device)
        return r.dist, out["features"][0].permute(1, 2, 0)

    def render(self, batch, render_contact_type=None):
        kind = self.render_contact_type if render_contact_type is None else render_contact_type
        pred = composite_pred(self.hand_model, self.obj_model, batch)
        rc = lambda camera, rtype, *a, **k: render_contacts(pred, batch, camera, rtype, *a, **dict(self.kw, **k))

        def hand_pair():      # 'hand_only' and 'accumulated': the canonical hand through the canonical camera, twice
            if not self.share_binning:
                h_dist, h_cmap = rc(batch["cano_camera"], "hand_only")
                _, acc_h_cmap = rc(batch["cano_camera"], "accumulated", acc_dist=self._accumulate(h_dist))
                return h_cmap, acc_h_cmap
            first, h_cmap = self._first_of_pair(pred, batch, batch["cano_camera"], "hand_only")
            _, acc_h_cmap = self._second_of_pair(pred, batch, batch["cano_camera"], first, "accumulated",
                                                 acc_dist=self._accumulate(first.dist))
            return h_cmap, acc_h_cmap

        rendered = None
        if kind == "gt_eval":
            h_cmap, acc_h_cmap = hand_pair()
            panels = [h_cmap, acc_h_cmap]
        elif kind == "acc_gt_eval":
            if self.acc_contacts is None:
                raise ValueError("'acc_gt_eval' colours the recorded sum `acc_contacts`")
            if self.share_binning:
                first, acc_h_cmap = self._first_of_pair(pred, batch, batch["camera"], "acc_gt_eval", "gray", 0, self.acc_contacts)
                _, skin_wts = self._second_of_pair(pred, batch, batch["camera"], first, "skin_wts", "gray", 0, None)
            else:
                _, acc_h_cmap = rc(batch["camera"], "acc_gt_eval", "gray", 0, self.acc_contacts)
                _, skin_wts = rc(batch["camera"], "skin_wts", "gray", 0, None)
            panels = [skin_wts, acc_h_cmap]
        elif kind == "results":
            rendered = self._rgb(pred, batch)
            _, o_cmap = rc(batch["camera"], "object_only")
            h_cmap, acc_h_cmap = hand_pair()
            panels = [rendered["render"], h_cmap, o_cmap, acc_h_cmap]
        elif kind == "nocs":
            rendered = self._rgb(pred, batch)
            _, o_cmap = rc(batch["camera"], "nocs_object_only")
            _, h_cmap = rc(batch["cano_camera"], "nocs_hand_only")
            panels = [rendered["render"], h_cmap, o_cmap]
        else:
            raise ValueError("render_contact_type is 'gt_eval', 'acc_gt_eval', 'results' or 'nocs', got %r" % (kind,))
        pred["render"] = torch.cat(panels, dim=1)
        pred["rendered"] = rendered
        return pred
