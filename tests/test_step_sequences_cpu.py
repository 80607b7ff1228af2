"""The coverage condition of tests/step_sequences.py, checked without a GPU: the committed sequences together contain every
transition of REQUIRED (views, model, transforms, targets, image-loss route, map terms, LPIPS, gradient outputs, skin grid,
interleaved calls, run lists -- each in both directions where it has two), every sequence stays within its step cap, and the
scripted sequence alone contains all of the flag transitions E-H."""
import step_sequences as S


def test_the_sequences_together_contain_every_transition():
    seen = set()
    for seq in S.sequences().values():
        seen |= S.transitions(seq)
    assert not (S.REQUIRED - seen), sorted(S.REQUIRED - seen)


def test_the_scripted_sequence_alone_contains_the_flag_transitions():
    seen = S.transitions(S.scripted())
    need = {t for t in S.REQUIRED if t[0] in "EFGH"}
    assert len(need) >= 28
    assert not (need - seen), sorted(need - seen)
    # ... and, but for the composite scene, everything else as well
    assert S.REQUIRED - seen == {"B:composite"}, sorted(S.REQUIRED - seen)


def test_step_caps_and_the_fixed_settings():
    seqs = S.sequences()
    assert seqs["scripted"]["cap"] == 48 and sum(1 for n in seqs if n.startswith("random-")) == 4
    for name, seq in seqs.items():
        assert 2 <= len(seq["steps"]) <= seq["cap"] <= 48, name
        assert name == "scripted" or seq["cap"] <= 32, name
        for st in seq["steps"]:
            assert set(st["flags"]) == set(S.FLAG_DEFAULTS), name
            assert all(0 <= v < S.N_CAMERAS for v in st["views"]) and len(set(st["views"])) == len(st["views"]), name
            assert "depth_cut" not in st["flags"]                      # stays off: its history dependence has its own tests
    assert sorted(s["loss"] for n, s in seqs.items() if n.startswith("random-")) == ["l1", "l1+ssim", "l1+ssim", "l1+ssim"]
    assert all(s["loss"] == "l1+ssim" for n, s in seqs.items() if not n.startswith("random-"))
    assert [n for n, s in seqs.items() if s["kind"] == "composite"] == ["random-2-composite"] and seqs["random-2-composite"]["n"] == 263
    f16 = seqs["fp16-constant-flags"]
    assert f16["sh_storage"] == "fp16" and len({S.flag_key(st)[:-1] for st in f16["steps"]}) == 1
    obj = seqs["object"]
    assert obj["kind"] == "object"
    for st in obj["steps"]:                                            # an object scene has no pose, skin or map flags
        assert st["flags"]["maps"] == "off" and not st["flags"]["pose_grad"] and not st["flags"]["skin_grid_grad"]
        assert not any(e in S.HAND_ONLY_EVENTS for e, _ in st["events"])


def test_the_sequences_leave_room_for_the_selective_fills():
    """The seeds are chosen so that a walk does not spend its steps on full fills (another V or N every step, a map term left
    on): by the host-side estimate at least a third of every sequence's steps can fill row-selectively."""
    for name, seq in S.sequences().items():
        st = seq["steps"]
        n = sum(S.may_engage(a, b) for a, b in zip(st[:-1], st[1:]))
        assert 3 * n >= len(st), (name, n, len(st))


def test_sequences_replay_exactly():
    a, b = S.sequences(), S.sequences()
    assert a == b
    seeds = [s for seq in a.values() for st in seq["steps"] for _, s in st["events"]]
    assert len(seeds) > 100


def test_transitions_of_a_pair_of_steps():
    p = S._step((0, 1, 2), {})
    q = S._step((0, 1, 2), dict(target_map=False), [("jitter", 1)], run_lists=0)
    assert S.step_transitions(p, q) == {"A:same", "E:target_map:T>F", "B:jitter", "K:run_lists:1>0"}
    r = S._step((3, 4, 5), dict(target_map=False, overlap_loss=False), sync_check=False)
    assert S.step_transitions(q, r) == {"A:other_ids", "E:overlap_route:T>F", "K:run_lists:0>1", "J:sync_check:T>F"}
