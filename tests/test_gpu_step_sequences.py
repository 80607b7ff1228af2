"""GPU: a training step's output is a function of the current model, views, targets and flags -- never of the steps before.

Every sequence of tests/step_sequences.py runs in two passes.  Pass 1 (reference): for every step a FRESH
HipViewCompute(persistent_grads=False) built from copies of the current leaves, grid, transforms and targets, the step's flags
given to the constructor; clones of every tensor of its output dict and of `last_image` are kept.  Pass 2 (live), after
`context.clear()`: ONE default-constructed object (kept buffers) goes through the same steps and the same seeded events, its
flags flipped as plain attributes, and every tensor must equal the reference bit for bit and be finite.  The reference never
runs between two live steps, so the live object's workspace chain (rows_seq / rows_owner / img_owner) is its own.

Not bitwise, by an existing test's statement: the loss scalar of loss="l1" is summed with float atomics -- 1e-6 absolute
(tests/test_gpu_fused.py::check_fused_run_to_run_determinism).  Nothing else has a tolerance.  The preflight of pass 1 (two fresh
objects per distinct flag combination must give equal bits) fails the test for any other quantity that is not reproducible.

Positive controls.  The scene gets one inert Gaussian: no point lies behind all twelve cameras of the rig (they surround the
hand) and a point outside the skin grid has no skin weights, so it sits among the others with opacity sigmoid(-40) -- below the
blend's 1/255 threshold everywhere, so no view ever gives it a gradient and its row is never active (asserted on every
reference step).  After each live step a sentinel is planted through `.data` (no version-counter change) in that row of the
`_xyz` gradient and -- when the next step's image loss does not read under empty tiles (the sparse rows loss without LPIPS) -- in
one pixel of the top row of tiles, which is empty in every reference image and where the targets equal the background (that
loss reads a span unless every tile over it is empty and the target is the background there).  A sentinel that survives the
next step proves the selective fill ran (`engaged`); it must be gone after everything that has to be answered by a full fill.
Every fifth Gaussian starts 6 logits further from zero, so that the jitter's sign flips take rows out of every view and back.

Sizes: 3000 Gaussians (263 for the composite) + the inert one, 96x64, grid_res 24, twelve cameras, stand-in LPIPS weights."""
import numpy as np
import pytest
import torch

import lpips_ref as R
import step_sequences as S
from util import max_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = 96, 64
BAR = 1e-4                      # fused against modular with LPIPS / a map term on (test_gpu_lpips_step.py, test_gpu_map_loss.py)
L1_LOSS_BAR = 1e-6              # tests/test_gpu_fused.py::check_fused_run_to_run_determinism ("summed with float atomics")
SENT_ROW, SENT_PIX = 777.0, 0.125
INERT_OPACITY = -40.0
W_LPIPS, W_MASK, W_DEPTH = 0.1, 0.5, 0.25


def lpips_net():
    from manus_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(*R.state_dicts("vgg", R.make_weights("vgg", 0)), net="vgg")      # test_gpu_lpips_step.net's weights


def rect_table(which):
    """The host table (12,4) of LPIPS windows: "A" two sizes, "B" three other sizes (equal sizes batch under lpips_batch)."""
    if which is None:
        return None
    sizes = {"A": [(40, 30), (32, 24)], "B": [(56, 40), (36, 28), (44, 32)]}[which]
    rows = []
    for v in range(S.N_CAMERAS):
        w, h = sizes[v % len(sizes)]
        rows.append(((7 * v) % (W - w + 1), (5 * v) % (H - h + 1), w, h))
    return np.asarray(rows, dtype=np.int32)


def bars_of(seq):
    return {"loss": L1_LOSS_BAR} if seq["loss"] == "l1" else {}


# ---------------------------------------------------------------------------------------------------------------------
# the state a sequence acts on
# ---------------------------------------------------------------------------------------------------------------------
class World:
    """Leaves, skin grid, transforms and targets of one pass, and the events on them.  Pass 1: plain tensors, copied into a
    fresh compute object per step.  Pass 2 (`live` set): the live object's own tensors, changed the way a training run changes
    them (in place + the notification the engine asks for)."""

    def __init__(self, seq):
        from manus_amd.synthetic import camera_table, make_scene
        sc = make_scene(n_gaussians=seq["n"], kind=seq["kind"], seed=6, grid_res=24, n_cameras=S.N_CAMERAS, width=W, height=H,
                        cam_radius=1.6, sigma_range=(2e-3, 8e-3), device="cpu")   # (1.6: the hand leaves the top row of tiles empty in every view)
        n = sc["params"]["_xyz"].shape[0]
        params = {k: torch.cat([v, v[n - 1:n]]) for k, v in sc["params"].items()}       # the inert Gaussian, appended
        op = params["_opacity"]                  # every fifth Gaussian far from the blend's 1/255 threshold (logit -5.5): the
        op[::5] = torch.sign(op[::5]) * (op[::5].abs() + 6.0)   # jitter's sign flips take such rows out of every view and back
        op[n] = INERT_OPACITY
        self.kind, self.sentinel, self.n_hand = seq["kind"], n, {"hand": n + 1, "composite": int(sc["n_hand"]), "object": 0}[seq["kind"]]
        self.ct = camera_table(sc["cameras"], DEV)
        self.base = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sc.items() if k not in ("params", "grid", "transforms")}
        self.params = {k: v.to(DEV) for k, v in params.items()}
        self.hand = sc.get("grid") is not None
        self.grid = sc["grid"].to(DEV).contiguous() if self.hand else None              # (D,H,W,B), the reference's layout
        self.transforms = sc["transforms"].to(DEV).contiguous()
        g = torch.Generator().manual_seed(17)
        self.targets = self._targets(g)
        self.masks = (torch.rand((S.N_CAMERAS, H, W), generator=g) * 3 - 1).clamp(0, 1).to(DEV)
        self.depths = (1.4 + 0.4 * torch.rand((S.N_CAMERAS, H, W), generator=g)).to(DEV)
        if self.hand:
            c, s = self.base["grid_center"].float(), self.base["grid_scale"].float()
            self.lo, self.hi = (c - 0.9 * s).reshape(1, 3), (c + 0.9 * s).reshape(1, 3)
        self.live = None
        self.last_out = None

    @staticmethod
    def _targets(g):
        """Seeded targets (V_all,3,H,W) that equal the background over the top row of tiles: there, under empty tiles, the
        sparse rows loss reads neither image (its spans are "identical") -- where the pixel sentinel is planted."""
        t = torch.rand((S.N_CAMERAS, 3, H, W), generator=g)
        t[:, :, :16] = 1.0
        return t.to(DEV)

    # -- current state ------------------------------------------------------------------------------------------------
    def P(self):
        return self.live.params if self.live is not None else self.params

    def scene(self, copy=True):
        cp = (lambda t: t.detach().clone()) if copy else (lambda t: t)
        sc = dict(self.base, params={k: v.detach().clone() for k, v in self.P().items()}, n_hand=self.n_hand)
        if self.hand:
            sc["grid"] = self.live.grid.dense() if self.live is not None else self.grid.clone()
            sc["transforms"] = cp(self.transforms)
        return sc

    def compute(self, seq, step, net, fused=True, persistent=False):
        """A fresh object of the current state with the step's flags given to the constructor."""
        from manus_amd.engine import HipViewCompute
        f = step["flags"]
        kw = dict(loss=seq["loss"], sh_storage=seq["sh_storage"], fused=fused, persistent_grads=persistent, depth_cut=False, ssim=f["ssim"],
                  sparse_loss=f["sparse_loss"], overlap_loss=f["overlap_loss"], pose_grad=f["pose_grad"], skin_grid_grad=f["skin_grid_grad"],
                  lpips_rects=rect_table(f["lpips_rects"]), lpips_norm=f["lpips_norm"], lpips_cache_targets=f["lpips_cache_targets"],
                  lpips_batch=f["lpips_batch"])
        if f["lpips_on"]:
            kw.update(lpips=net, w_lpips=W_LPIPS)
        if f["maps"] != "off":
            kw.update(mask_targets=self.masks.clone(), w_mask=W_MASK)
        if f["maps"] == "mask+depth":
            kw.update(depth_targets=self.depths.clone(), w_depth=W_DEPTH)
        hc = HipViewCompute(self.scene(), self.targets.clone(), self.ct, **kw)
        hc.target_map, hc.attach_list, hc.sync_check = f["target_map"], f["attach_list"], step["sync_check"]   # (no constructor arguments)
        return hc

    def make_live(self, seq, net):
        """The default-constructed object of pass 2; the world's transforms and targets are the tensors it reads."""
        from manus_amd.engine import HipViewCompute
        self.live = None
        sc = self.scene(copy=False)
        if self.hand:
            sc["grid"] = self.grid.clone()
        live = HipViewCompute(sc, self.targets, self.ct, loss=seq["loss"], sh_storage=seq["sh_storage"], lpips=net, w_lpips=W_LPIPS)
        assert live.persistent_grads and not live.depth_cut and live.fused
        live.lpips_on = False
        self.live, self.params, self.grid = live, None, None
        return live

    def set_flags(self, step):
        """The step's flags on the live object: plain attributes, flipped as a Trainer or a caller would."""
        live, f = self.live, step["flags"]
        for name in ("ssim", "sparse_loss", "target_map", "attach_list", "overlap_loss", "pose_grad", "skin_grid_grad", "lpips_on",
                     "lpips_norm", "lpips_cache_targets", "lpips_batch"):
            setattr(live, name, f[name])
        live.lpips_rects = rect_table(f["lpips_rects"])
        live.sync_check = step["sync_check"]
        if f["maps"] != "off" and live.mask_targets is None:
            live.mask_targets = self.masks
        if f["maps"] == "mask+depth" and live.depth_targets is None:
            live.depth_targets = self.depths
        live.w_mask = W_MASK if f["maps"] != "off" else 0.0
        live.w_depth = W_DEPTH if f["maps"] == "mask+depth" else 0.0

    # -- events -------------------------------------------------------------------------------------------------------
    def _clamp(self, xyz):
        if self.hand:       # articulated rows stay inside the skin grid (outside it a Gaussian has no weights: 0 / 0)
            na = self.n_hand
            xyz[:na].copy_(torch.max(torch.min(xyz[:na], self.hi.to(xyz.device)), self.lo.to(xyz.device)))

    def _resize(self, new, n_hand):
        from manus_amd import rasterizer as rz
        self.n_hand = n_hand
        if self.live is None:
            self.params = new
        else:               # as Trainer.train_step does after a densification / pruning
            self.live.set_params(new, n_hand if self.kind == "composite" else None)
            rz.context(DEV).clear()

    def apply(self, name, seed, seq, step):
        from manus_amd import rasterizer as rz
        from manus_amd._lib import ManusHipError
        from manus_amd.engine import HipViewCompute
        g = torch.Generator().manual_seed(seed)
        live, P = self.live, self.P()
        N = P["_xyz"].shape[0]
        views, scale = list(step["views"]), step["scale"]
        if name == "jitter":            # positions jitter, a tenth of the Gaussians turn transparent / opaque
            noise = 0.004 * torch.randn((N, 3), generator=g)
            flip = torch.rand((N, 1), generator=g) < 0.1
            noise[self.sentinel], flip[self.sentinel] = 0.0, False
            noise, flip = noise.to(DEV), flip.to(DEV)
            with torch.no_grad():
                P["_xyz"].add_(noise)
                self._clamp(P["_xyz"])
                P["_opacity"][flip] = -P["_opacity"][flip]
            if live is not None:
                live.mark_params_changed()
        elif name == "grow":            # clones of seeded rows (static rows of a composite), moved a little, appended
            lo = self.n_hand if self.kind == "composite" else 0
            pool = [i for i in range(lo, N) if i != self.sentinel]
            k = max(1, len(pool) // 19)
            idx = torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]].to(DEV)
            shift = (0.003 * torch.randn((k, 3), generator=g)).to(DEV)
            with torch.no_grad():
                new = {n_: torch.cat([v.detach(), v.detach()[idx]]) for n_, v in P.items()}
                new["_xyz"][N:] += shift
            n_hand = self.n_hand + (k if self.kind == "hand" else 0)
            self._resize(new, n_hand)
            with torch.no_grad():
                self._clamp(self.P()["_xyz"])
        elif name == "shrink":          # seeded rows removed, the order of the others kept
            pool = [i for i in range(N) if i != self.sentinel]
            k = max(1, len(pool) // 14)
            drop = torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]]
            keep = torch.ones(N, dtype=torch.bool)
            keep[drop] = False
            self.sentinel = int(keep[:self.sentinel].sum())
            n_hand = int(keep[:self.n_hand].sum())
            kd = keep.to(DEV)
            self._resize({n_: v.detach()[kd].clone() for n_, v in P.items()}, n_hand)
        elif name in ("transforms_inplace", "transforms_data"):
            d = (0.003 * torch.randn(tuple(self.transforms.shape[:2]) + (3,), generator=g)).to(DEV)
            if name == "transforms_inplace":        # torch sees it: the version counter moves
                self.transforms[:, :, :3, 3].add_(d)
            else:                                   # a write torch does not see, announced like pose.PoseRefiner.apply does
                self.transforms.data[:, :, :3, 3].add_(d)
                if live is not None:
                    live.transforms_changed()
        elif name == "targets_set":
            self.targets = self._targets(g)
            if live is not None:
                live.targets = self.targets
        elif name == "targets_inplace":
            self.targets.mul_(0.75).add_(0.25 * self._targets(g))       # (the top band stays 0.75 + 0.25 = the background)
        elif name == "targets_data":                # a kernel given the raw pointer (frames.FrameStore), announced
            self.targets.data.copy_(self._targets(g))
            if live is not None:
                live.view_constants_changed()
        elif name == "skin_grid":                   # the refiner's entry point: a write through the pointer, then bump()
            shape = tuple(self.grid.shape) if live is None else (live.grid.D, live.grid.H, live.grid.W, live.grid.B)
            f = (1.0 + 0.2 * (torch.rand(shape, generator=g) - 0.5)).to(DEV)
            if live is None:
                self.grid.mul_(f)
            else:
                v0 = live.grid.version
                live.grid.data.data[..., :live.grid.B].mul_(f)
                assert live.grid.version == v0
                live.grid.bump()
                assert live.grid.version == v0 + 1
        elif live is None:
            pass                                    # the interleaved calls below touch the live object alone
        elif name == "fwd_only":                    # other views, the same V: the forward of the same pooled workspace
            other = [int(v) for v in torch.randperm(S.N_CAMERAS, generator=g)[:len(views)]]
            with torch.no_grad():
                live.forward_views_fused(other)
        elif name == "pairs":
            assert len(live.pairs_per_view()) == S.N_CAMERAS
        elif name == "other_object":                # a step of a second object on the same pooled workspace
            second = HipViewCompute(self.scene(), self.targets.clone(), self.ct, loss=seq["loss"], sh_storage=seq["sh_storage"])
            second(views, scale)
        elif name == "scribble":                    # the caller writes into what it was handed (torch sees it)
            if self.last_out is not None:
                o = self.last_out
                o["grads"]["_xyz"].add_(1.0)
                o["grads"]["_features_rest"][:, 3].fill_(7.0)
                o["grad2d"].fill_(5.0)
                o["vis"].zero_()
                live.last_image.mul_(0.25)
        elif name == "raise":                       # a step that raises after its forward (test_failed_step_leaves_the_kept_loss_workspace_clean)
            ctx = rz.context(DEV)
            real, calls = ctx.forward, []

            def forward_then_fail(*a, **k):
                r = real(*a, **k)
                if not calls:
                    calls.append(1)
                    raise ManusHipError("injected failure after the forward")
                return r

            ctx.forward = forward_then_fail
            try:
                with pytest.raises(ManusHipError, match="injected"):
                    live(views, scale)
            finally:
                del ctx.forward
            assert calls and ctx.forward == real
        else:
            raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# one step, its tensors, the comparison
# ---------------------------------------------------------------------------------------------------------------------
def run_step(hc, step):
    from manus_amd import rasterizer as rz
    from manus_amd._lib import lib
    prev = lib().mgr_views_backward_run_lists(step["run_lists"])
    try:
        out = hc(list(step["views"]), step["scale"])
    finally:
        lib().mgr_views_backward_run_lists(prev)
    rz.context(DEV).poll()             # (sync_check False leaves a fence: an overflow would raise here)
    return out


def tensors_of(out, hc):
    """Clones of every tensor of the output dict and of `last_image`, by name."""
    t = {}
    for k, v in out.items():
        if k == "grads":
            for n, g in v.items():
                t["grads." + n] = g.detach().clone()
        elif k == "d_skin_grid":
            vox, rows = v.rows()
            t["d_skin_grid.count"], t["d_skin_grid.voxel"], t["d_skin_grid.grad"] = v.count.clone(), vox.clone(), rows.clone()
        elif k == "overflow":
            assert int(v.reshape(-1)[0]) == 0
        elif torch.is_tensor(v):
            t[k] = v.detach().clone()
    t["last_image"] = hc.last_image.detach().clone()
    return t


def mismatches(ref, got, bars, what):
    """Names whose tensors are not bit for bit equal (beyond the documented bars), with a figure; finiteness of `got`."""
    bad = []
    if set(ref) != set(got):
        return ["%s: outputs %s against %s" % (what, sorted(got), sorted(ref))]
    for k, r in ref.items():
        x = got[k]
        if x.is_floating_point() and not bool(torch.isfinite(x).all()):
            bad.append("%s: %s is not finite" % (what, k))
        elif x.shape != r.shape or x.dtype != r.dtype:
            bad.append("%s: %s is %s %s against %s %s" % (what, k, tuple(x.shape), x.dtype, tuple(r.shape), r.dtype))
        elif not torch.equal(x, r):
            d = float((x.double() - r.double()).abs().max())
            if k in bars and d <= bars[k]:
                continue
            n = int((x != r).sum())
            bad.append("%s: %s differs in %d of %d entries, max |diff| %.3e (max |ref| %.3e)" % (what, k, n, r.numel(), d, float(r.double().abs().max())))
    return bad


def reference_pass(seq):
    """Pass 1.  -> per step the reference tensors; the empty tile; the row sets; preflight fall-backs."""
    world, net = World(seq), lpips_net()
    refs, seen, fallbacks, rowsets = [], set(), set(), set()
    empty = torch.ones(((H + 15) // 16, (W + 15) // 16), dtype=torch.bool, device=DEV)
    for k, step in enumerate(seq["steps"]):
        for name, seed in step["events"]:
            world.apply(name, seed, seq, step)
        hc = world.compute(seq, step, net)
        ref = tensors_of(run_step(hc, step), hc)
        bad = [m for m in mismatches(ref, ref, {}, "%s step %d reference" % (seq["name"], k))]
        assert not bad, bad
        s = world.sentinel                         # the inert Gaussian: never a gradient, in any view
        assert all(float(v[s].abs().sum()) == 0.0 for n, v in ref.items() if n.startswith("grads.")) and float(ref["grad2d"][s]) == 0.0
        rowsets.add((ref["grads._xyz"].shape[0], ref["grads._xyz"].abs().sum(1).ne(0).cpu().numpy().tobytes()))
        bg = world.base["bg"].reshape(1, 3, 1, 1)
        at_bg = (ref["last_image"] == bg).all(1).all(0)                     # (H,W): every view shows the background here
        pad = torch.ones((empty.shape[0] * 16, empty.shape[1] * 16), dtype=torch.bool, device=DEV)
        pad[:H, :W] = at_bg
        empty &= pad.reshape(empty.shape[0], 16, empty.shape[1], 16).all(3).all(1)
        key = S.flag_key(step)
        if key not in seen:                        # preflight: two fresh objects of this flag combination, equal bits
            seen.add(key)
            hc2 = world.compute(seq, step, net)
            again = tensors_of(run_step(hc2, step), hc2)
            strict = mismatches(ref, again, {}, "%s step %d preflight" % (seq["name"], k))
            loose = mismatches(ref, again, bars_of(seq), "%s step %d preflight" % (seq["name"], k))
            for m in strict:
                print("not reproducible between two fresh objects:", m)
            assert not loose, loose                # no existing test documents these as not bitwise: a finding
            fallbacks |= {m.split(": ")[1].split(" ")[0] for m in strict}
        if k in seq["anchors"]:
            anchor(world, seq, step, net, ref, k)
        refs.append(ref)
    # the top ROW of tiles, empty from edge to edge in every view of every step: the sparse rows loss leaves a span unread
    # only where every tile over it is empty and the target is the background (`World._targets`), and a span is as wide as
    # these frames
    return refs, ([0, 0] if bool(empty[0].all()) else None), rowsets, fallbacks


def anchor(world, seq, step, net, ref, k):
    """The same state on the modular route (fused=False), judged with the bars of the tests that compare the two routes."""
    f = step["flags"]
    mod = world.compute(seq, step, net, fused=False)
    om = run_step(mod, step)
    strict = f["lpips_on"] or f["maps"] != "off"
    a, b = float(ref["loss"]), float(om["loss"])
    print("%s step %d anchor: loss fused %.7e modular %.7e" % (seq["name"], k, a, b))
    assert abs(a - b) <= BAR * abs(b), (k, a, b)
    for name in ("loss_lpips", "loss_mask", "loss_depth", "loss_ssim"):
        assert (name in om) == (name in ref), (k, name)
        if name in om:
            assert abs(float(ref[name]) - float(om[name])) <= BAR * max(abs(float(om[name])), 1e-30), (k, name)
    for name, g in om["grads"].items():
        x, y = ref["grads." + name].cpu().numpy().astype(np.float64), g.detach().cpu().numpy().astype(np.float64)
        e = max_rel_err(x, y)
        print("%s step %d anchor: %-16s fused against modular %.3g" % (seq["name"], k, name, e))
        if strict:                                 # BAR of test_gpu_lpips_step.py / test_gpu_map_loss.py
            assert e < BAR, (k, name, e)
        else:                                      # tests/test_gpu_fused.py::check_fused_equals_modular
            assert e < 5e-3, (k, name, e)
            rows = np.abs(x - y).reshape(x.shape[0], -1).max(1) > 2e-5 * np.abs(y).max()
            assert rows.mean() < 0.03, (k, name, rows.sum())
    assert torch.equal(ref["vis"], om["vis"])
    if f["maps"] == "off":                         # (the modular route's grad2d includes the map term: DESIGN.md section 9)
        assert max_rel_err(ref["grad2d"].cpu().numpy(), om["grad2d"].cpu().numpy()) < (BAR if strict else 5e-3)


def pixel_safe(seq, step):
    """The step's image loss does not read the image under a row of empty tiles (the sparse rows loss; LPIPS reads the whole frame)."""
    f = step["flags"]
    return seq["loss"] == "l1+ssim" and f["ssim"] == "rows" and f["sparse_loss"] and not f["lpips_on"]


def must_refill(prev, step):
    """(rows, image): the step has to answer what happened since the step before with a full fill.  Both after a
    torch-visible write, another object's step on the workspace, a raised step and a change of N or V; the rows alone on and
    after a step with a map term on or with more than 8 views (the kept image depends on neither: the maps are rendered into
    buffers of their own, and the forward has no view groups)."""
    hard = any(n in ("scribble", "other_object", "raise", "grow", "shrink") for n, _ in step["events"]) or len(prev["views"]) != len(step["views"])
    soft = any(s["flags"]["maps"] != "off" or len(s["views"]) > 8 for s in (prev, step))
    return hard or soft, hard


def live_pass(seq, refs, tile):
    """Pass 2.  -> (mismatches, rows engaged per step, image engaged per step)."""
    from manus_amd import rasterizer as rz
    world, net = World(seq), lpips_net()
    rz.context(DEV).clear()
    live = world.make_live(seq, net)
    steps, bars = seq["steps"], bars_of(seq)
    bad, rows_on, img_on = [], [], []
    planted_pix = False
    py, px = (tile[0] * 16 + 8, tile[1] * 16 + 8) if tile is not None else (None, None)
    bg = world.base["bg"]
    for k, step in enumerate(steps):
        world.set_flags(step)
        for name, seed in step["events"]:
            world.apply(name, seed, seq, step)
        out = run_step(live, step)
        got = tensors_of(out, live)
        s = world.sentinel
        row = got["grads._xyz"][s]
        r_on = k > 0 and bool((row == SENT_ROW).all())
        if r_on:                                   # the row was not written: the selective fill ran.  What it left is ours
            row.zero_()
        pix = got["last_image"][0, :, py, px] if planted_pix else None
        i_on = planted_pix and bool((pix == SENT_PIX).all())
        if i_on:
            pix.copy_(bg)
        rows_on.append(r_on)
        img_on.append(i_on)
        if k > 0:
            need_rows, need_img = must_refill(steps[k - 1], step)
            assert not (need_rows and r_on), "%s step %d: the gradient rows were not filled in full" % (seq["name"], k)
            assert not (need_img and i_on), "%s step %d: the image was not written in full" % (seq["name"], k)
        bad += mismatches(refs[k], got, bars, "%s step %d %s" % (seq["name"], k, sorted(S.step_transitions(steps[k - 1], step)) if k else []))
        # the sentinels for the next step (`.data`: the version counters do not move)
        world.last_out = out
        v0 = out["grads"]["_xyz"]._version
        out["grads"]["_xyz"].data[s] = SENT_ROW
        planted_pix = tile is not None and k + 1 < len(steps) and pixel_safe(seq, steps[k + 1])
        if tile is not None:                       # (a sentinel that survived is taken out again when the next step would read it)
            live.last_image.data[0, :, py, px] = SENT_PIX if planted_pix else bg
        assert out["grads"]["_xyz"]._version == v0 and not live._kept.touched()
    rz.context(DEV).clear()
    return bad, rows_on, img_on


def run_sequence(name):
    from manus_amd import rasterizer as rz
    from manus_amd._lib import lib
    seq = S.sequences()[name]
    rz.context(DEV).clear()
    run_lists = lib().mgr_views_backward_run_lists(1)
    try:
        refs, tile, rowsets, fallbacks = reference_pass(seq)
        assert len(rowsets) > 1, "the set of rows with a gradient never changed"
        bad, rows_on, img_on = live_pass(seq, refs, tile)
    finally:
        lib().mgr_views_backward_run_lists(run_lists)
        rz.context(DEV).clear()
    print("%s: %d steps, %d with the selective row fill engaged, %d with the kept image engaged (empty tile %s); not bitwise between fresh objects: %s"
          % (name, len(seq["steps"]), sum(rows_on), sum(img_on), tile, sorted(fallbacks) or "nothing"))
    print("%s: rows engaged %s" % (name, "".join("x" if e else "." for e in rows_on)))
    print("%s: image engaged %s" % (name, "".join("x" if e else "." for e in img_on)))
    for m in bad:
        print(m)
    assert not bad, "%d mismatches, the first: %s" % (len(bad), bad[0])
    return seq, rows_on, img_on, tile


def test_scripted_sequence():
    """The scripted trainer life: every transition in one run; three steps anchored to the modular route; the engagement side
    of the positive controls -- every flag transition of E-H happens at least once directly after a step on which a selective
    fill provably ran (the rows', or for the steps behind a map term, which fills the rows in full by design, the image's), and
    the selective row fill ran on at least a third of the steps."""
    seq, rows_on, img_on, tile = run_sequence("scripted")
    assert tile is not None, "no image tile is empty in every reference image"
    steps = seq["steps"]
    after_engaged = set()
    for k in range(1, len(steps)):
        if rows_on[k - 1] or img_on[k - 1]:
            after_engaged |= S.step_transitions(steps[k - 1], steps[k])
    need = {t for t in S.REQUIRED if t[0] in "EFGH"}
    assert not (need - after_engaged), sorted(need - after_engaged)
    assert 3 * sum(rows_on) >= len(steps), (sum(rows_on), len(steps))


@pytest.mark.parametrize("name", ["random-1", "random-2-composite", "random-3-l1", "random-4", "fp16-constant-flags", "object"])
def test_sequence(name):
    run_sequence(name)
