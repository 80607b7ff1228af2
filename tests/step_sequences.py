"""Sequences of training steps of ONE `HipViewCompute`, as data (host only: no torch, no GPU).

A step's output must be a function of the current model, views, targets and flags -- never of what ran before.  The sequences
here walk one compute object through everything a training run does to it between two steps; tests/test_gpu_step_sequences.py
replays each of them twice (a fresh object per step, then one kept object) and compares bits, and
tests/test_step_sequences_cpu.py checks that the sequences together contain every transition named in REQUIRED.

A step is a dict:
    views       tuple of view ids out of the pool of N_CAMERAS cameras
    scale       the step's loss scale
    flags       the flag values of the step (FLAG_DEFAULTS lists the axes: E image-loss route, F map terms, G LPIPS, H gradient outputs)
    run_lists   the library's mgr_views_backward_run_lists switch during the step (K), set the same way in both passes
    sync_check  the compute object's `sync_check` during the step (J)
    events      what happens BEFORE the step, in order: (name, seed) pairs.  An event draws whatever it needs from a generator
                seeded with its seed alone, never from a step's output, so a sequence replays exactly.

A sequence is a dict: name, kind ("hand" | "composite" | "object"), n (Gaussians), loss, sh_storage, steps, cap (the most steps
it may have), anchors (step indices that are also run on the modular route)."""
import random

N_CAMERAS = 12

FLAG_DEFAULTS = dict(
    ssim="rows", sparse_loss=True, target_map=True, attach_list=True, overlap_loss=True,          # E
    maps="off",                                                                                   # F: "off" | "mask" | "mask+depth"
    lpips_on=False, lpips_rects=None, lpips_cache_targets=False, lpips_batch=0, lpips_norm="frame",   # G (rects: None | "A" | "B")
    pose_grad=False, skin_grid_grad=False)                                                        # H

AXIS_GROUP = dict(ssim="E", sparse_loss="E", target_map="E", attach_list="E", overlap_loss="E", maps="F", lpips_on="G",
                  lpips_rects="G", lpips_cache_targets="G", lpips_batch="G", lpips_norm="G", pose_grad="H", skin_grid_grad="H")

# events: B model, C transforms, D targets, I skin grid, J interleaved calls
MODEL_EVENTS = ("jitter", "grow", "shrink")
TRANSFORM_EVENTS = ("transforms_inplace", "transforms_data")
TARGET_EVENTS = ("targets_set", "targets_inplace", "targets_data")
GRID_EVENTS = ("skin_grid",)
CALL_EVENTS = ("fwd_only", "pairs", "other_object", "scribble", "raise")
EVENT_GROUP = dict([(e, "B") for e in MODEL_EVENTS] + [(e, "C") for e in TRANSFORM_EVENTS] + [(e, "D") for e in TARGET_EVENTS]
                   + [(e, "I") for e in GRID_EVENTS] + [(e, "J") for e in CALL_EVENTS])
# what only an articulated scene has
HAND_ONLY_EVENTS = TRANSFORM_EVENTS + GRID_EVENTS
HAND_ONLY_AXES = ("maps", "pose_grad", "skin_grid_grad")


def _t(x):
    return {True: "T", False: "F", None: "None"}.get(x, str(x)) if isinstance(x, (bool, type(None))) else str(x)


def _required():
    req = {"A:same", "A:other_ids", "A:8>3", "A:3>8", "A:le8>11", "A:11>le8", "A:V=1", "B:composite"}
    req |= {"%s:%s" % (EVENT_GROUP[e], e) for e in EVENT_GROUP}
    for axis in ("sparse_loss", "target_map", "attach_list", "lpips_on", "lpips_cache_targets", "pose_grad", "skin_grid_grad"):
        req |= {"%s:%s:F>T" % (AXIS_GROUP[axis], axis), "%s:%s:T>F" % (AXIS_GROUP[axis], axis)}
    req |= {"E:ssim:rows>spatial", "E:ssim:spatial>rows", "E:overlap_route:F>T", "E:overlap_route:T>F"}
    req |= {"F:maps:off>mask", "F:maps:mask>mask+depth", "F:maps:mask+depth>off"}
    req |= {"G:lpips_rects:None>A", "G:lpips_rects:A>B", "G:lpips_rects:B>None", "G:lpips_batch:0>4", "G:lpips_batch:4>0",
            "G:lpips_norm:frame>window", "G:lpips_norm:window>frame"}
    req |= {"J:sync_check:T>F", "J:sync_check:F>T", "K:run_lists:1>0", "K:run_lists:0>1"}
    return frozenset(req)


REQUIRED = _required()


def step_transitions(prev, cur):
    """The transitions between two consecutive steps (labels of REQUIRED's kind; the events of `cur` included)."""
    out = set()
    a, b = tuple(prev["views"]), tuple(cur["views"])
    if a == b:
        out.add("A:same")
    elif len(a) == len(b):
        out.add("A:other_ids")
    if (len(a), len(b)) in ((8, 3), (3, 8)):
        out.add("A:%d>%d" % (len(a), len(b)))
    if len(a) <= 8 and len(b) == 11:
        out.add("A:le8>11")
    if len(a) == 11 and len(b) <= 8:
        out.add("A:11>le8")
    if len(b) == 1 and len(a) != 1:
        out.add("A:V=1")
    for axis, g in AXIS_GROUP.items():
        x, y = prev["flags"][axis], cur["flags"][axis]
        if x != y and axis != "overlap_loss":
            out.add("%s:%s:%s>%s" % (g, axis, _t(x), _t(y)))
    # the overlap route is what overlap_loss selects with the target maps off (and the sparse rows loss on)
    route = lambda s: s["flags"]["overlap_loss"] and not s["flags"]["target_map"]
    if route(prev) != route(cur) and not prev["flags"]["target_map"] and not cur["flags"]["target_map"]:
        out.add("E:overlap_route:%s>%s" % (_t(route(prev)), _t(route(cur))))
    if prev["sync_check"] != cur["sync_check"]:
        out.add("J:sync_check:%s>%s" % (_t(prev["sync_check"]), _t(cur["sync_check"])))
    if prev["run_lists"] != cur["run_lists"]:
        out.add("K:run_lists:%d>%d" % (prev["run_lists"], cur["run_lists"]))
    for name, _ in cur["events"]:
        out.add("%s:%s" % (EVENT_GROUP[name], name))
    return out


def transitions(seq):
    out = {"B:composite"} if seq["kind"] == "composite" else set()
    for prev, cur in zip(seq["steps"][:-1], seq["steps"][1:]):
        out |= step_transitions(prev, cur)
    return out


def may_engage(prev, cur):
    """Host-side estimate: can the row-selective fill of the backward run at `cur`?  It needs the rows the step before left on
    the same workspace: the same number of views (3 to 8: one and two views go through the plain gather, more than 8 through two
    view groups) and of Gaussians, no map term on either step, the run lists on for both, and nothing in between that takes the
    workspace or the buffers away.  (Used to keep the seeded walks from spending their steps on full fills; what did run
    selectively is measured on the GPU, with sentinels.)"""
    if len(prev["views"]) != len(cur["views"]) or not 3 <= len(cur["views"]) <= 8:
        return False
    if prev["flags"]["maps"] != "off" or cur["flags"]["maps"] != "off" or not (prev["run_lists"] and cur["run_lists"]):
        return False
    return not any(n in ("grow", "shrink", "other_object", "scribble", "raise") for n, _ in cur["events"])


def flag_key(step):
    """The step's flag combination (what the preflight of the reference pass counts as distinct)."""
    return tuple(sorted((k, str(v)) for k, v in step["flags"].items())) + (("V>8", len(step["views"]) > 8),)


def _step(views, flags, events=(), scale=None, run_lists=1, sync_check=True):
    assert all(0 <= v < N_CAMERAS for v in views) and len(set(views)) == len(views) and len(views) >= 1
    f = dict(FLAG_DEFAULTS)
    f.update(flags)
    assert set(f) == set(FLAG_DEFAULTS)
    return dict(views=tuple(views), scale=float(scale if scale is not None else 1.0 / len(views)), flags=f, run_lists=int(run_lists),
                sync_check=bool(sync_check), events=[(str(n), int(s)) for n, s in events])


# ---------------------------------------------------------------------------------------------------------------------
# the scripted "trainer life"
# ---------------------------------------------------------------------------------------------------------------------
def scripted():
    """Every transition of REQUIRED (but the composite scene) in one run.  The flag changes of E-H come first, on one view set
    and one N with the model moving under them, so that each happens on buffers the step before has kept; then the events
    that must NOT leave kept state behind (another V, another N, another object, a raised step ...)."""
    V4, W4 = (0, 1, 2, 3), (5, 6, 7, 8)
    S = []
    seed = [100]

    def add(flags=None, events=(), views=V4, **kw):
        ev = []
        for e in events:
            seed[0] += 1
            ev.append((e, seed[0]))
        cur = dict(S[-1]["flags"]) if S else dict(FLAG_DEFAULTS)
        cur.update(flags or {})
        S.append(_step(views, cur, ev, **kw))

    add()                                                                         # 0
    add(events=["jitter"])                                                        # 1   same views, the model moved (anchor)
    add(dict(ssim="spatial"))                                                     # 2
    add(dict(ssim="rows", sparse_loss=False), ["jitter"])                         # 3
    add(dict(sparse_loss=True, target_map=False))                                 # 4   the overlap route
    add(dict(overlap_loss=False), ["jitter"])                                     # 5   plain sparse route
    add(dict(overlap_loss=True))                                                  # 6   the overlap route again
    add(dict(target_map=True, attach_list=False), ["jitter"])                     # 7   the mapped list in a launch of its own
    add(dict(attach_list=True, pose_grad=True))                                   # 8
    add(dict(pose_grad=False, skin_grid_grad=True), ["jitter"])                   # 9
    add(dict(skin_grid_grad=False, lpips_on=True))                                # 10
    add(dict(lpips_rects="A"), ["jitter"])                                        # 11  (anchor)
    add(dict(lpips_rects="B", lpips_cache_targets=True))                          # 12
    add(dict(lpips_batch=4, lpips_norm="window"), ["jitter"])                     # 13
    add(dict(lpips_norm="frame", lpips_batch=0))                                  # 14
    add(dict(lpips_cache_targets=False, lpips_rects=None), ["jitter"])            # 15
    add(dict(lpips_on=False))                                                     # 16
    add(dict(maps="mask"), ["jitter"])                                            # 17
    add(dict(maps="mask+depth"))                                                  # 18  (anchor)
    add(dict(maps="off"), ["jitter"])                                             # 19
    add(events=["jitter"])                                                        # 20
    add(events=["transforms_inplace"])                                            # 21
    add(events=["transforms_data", "jitter"])                                     # 22
    add(events=["targets_set"])                                                   # 23
    add(events=["targets_inplace", "jitter"])                                     # 24
    add(events=["targets_data"])                                                  # 25
    add(dict(skin_grid_grad=True), ["skin_grid", "jitter"])                       # 26
    add(dict(skin_grid_grad=False), ["fwd_only"])                                 # 27
    add(events=["pairs", "jitter"])                                               # 28
    add(events=["other_object"])                                                  # 29
    add(events=["jitter"])                                                        # 30
    add(events=["scribble"])                                                      # 31
    add(events=["jitter"])                                                        # 32
    add(events=["raise"])                                                         # 33
    add(events=["jitter"], sync_check=False)                                      # 34
    add(sync_check=False)                                                         # 35
    add(events=["jitter"])                                                        # 36  sync_check on again
    add(run_lists=0)                                                              # 37
    add(events=["jitter"])                                                        # 38  run lists on again
    add(views=W4)                                                                 # 39  other ids, same V
    add(views=tuple(range(8)), events=["jitter"])                                 # 40
    add(views=(2, 9, 4))                                                          # 41  8 -> 3
    add(views=tuple(range(4, 12)), events=["jitter"])                             # 42  3 -> 8
    add(views=tuple(range(11)))                                                   # 43  -> 11: two view groups
    add(views=(1, 3, 5, 7, 9), events=["jitter"])                                 # 44  11 -> 5
    add(views=(6,))                                                               # 45  one view
    add(views=V4, events=["grow"])                                                # 46  N grows
    add(views=V4, events=["shrink", "jitter"])                                    # 47  N shrinks
    return dict(name="scripted", kind="hand", n=3000, loss="l1+ssim", sh_storage="fp32", steps=S, cap=48, anchors=(1, 11, 18))


# ---------------------------------------------------------------------------------------------------------------------
# seeded random sequences
# ---------------------------------------------------------------------------------------------------------------------
_VIEW_COUNTS = (1, 2, 3, 4, 4, 5, 8, 8, 11)


def random_sequence(name, seed, n_steps, kind="hand", n=3000, loss="l1+ssim", sh_storage="fp32", constant_flags=False, cap=32):
    """A seeded walk: per step maybe other views, one or two flag axes moved, a few events, the two switches."""
    rng = random.Random(seed)
    hand = kind != "object"
    axes = [a for a in FLAG_DEFAULTS if hand or a not in HAND_ONLY_AXES]
    events = [e for e in EVENT_GROUP if hand or e not in HAND_ONLY_EVENTS]
    choices = dict(ssim=("rows", "spatial"), maps=("off", "mask", "mask+depth"), lpips_rects=(None, "A", "B"), lpips_batch=(0, 4),
                   lpips_norm=("frame", "window"))
    flags, views, run_lists, sync = dict(FLAG_DEFAULTS), tuple(range(4)), 1, True
    steps = []
    for k in range(n_steps):
        ev = []
        if k:
            r = rng.random()
            if len(views) not in (3, 4, 5, 8) and r < 0.7:   # (view counts without a selective fill are not stayed at for long)
                views = tuple(rng.sample(range(N_CAMERAS), rng.choice((3, 4, 5, 8))))
            elif r < 0.15:                       # other ids, same V
                views = tuple(rng.sample(range(N_CAMERAS), len(views)))
            elif r < 0.30:                       # another V
                views = tuple(rng.sample(range(N_CAMERAS), rng.choice(_VIEW_COUNTS)))
            if not constant_flags and rng.random() < 0.7:
                for axis in rng.sample(axes, rng.choice((1, 1, 2))):
                    opts = [o for o in choices.get(axis, (False, True)) if o != flags[axis]]
                    flags[axis] = rng.choice(opts)
            elif flags["maps"] != "off" and rng.random() < 0.7:   # (nor is a map term, which fills in full, left on for long)
                flags["maps"] = "off"
            if rng.random() < 0.6:
                ev.append(("jitter", rng.randrange(1 << 30)))
            if rng.random() < 0.35:
                ev.append((rng.choice(events), rng.randrange(1 << 30)))
            if not constant_flags and rng.random() < 0.12:
                run_lists = 1 - run_lists
            if not constant_flags and rng.random() < 0.12:
                sync = not sync
        steps.append(_step(views, flags, ev, run_lists=run_lists, sync_check=sync))
    return dict(name=name, kind=kind, n=n, loss=loss, sh_storage=sh_storage, steps=steps, cap=cap, anchors=())


def sequences():
    """The committed sequences, by name."""
    seqs = [scripted(),
            random_sequence("random-1", 40, 24),
            random_sequence("random-2-composite", 25, 24, kind="composite", n=263),
            random_sequence("random-3-l1", 57, 24, loss="l1"),
            random_sequence("random-4", 49, 24),
            random_sequence("fp16-constant-flags", 55, 14, sh_storage="fp16", constant_flags=True),
            random_sequence("object", 13, 16, kind="object")]
    return {s["name"]: s for s in seqs}
