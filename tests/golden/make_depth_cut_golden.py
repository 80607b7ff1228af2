#!/usr/bin/env python3
"""Generate tests/golden/depth_cut_policy.json: a recorded run of the depth-cut policy of `HipViewCompute` on the CPU.

    python tests/golden/make_depth_cut_golden.py

The committed trace was produced by commit dc46d62, the last one in which the whole policy -- back-off state machine,
parking / restoring of the hint tables, the calls that set the library's margins -- was the single method
`HipViewCompute._cut_flag`.  tests/test_depth_cut_policy_cpu.py replays the same script through `drive()` below on the
code as it is now and asserts equality, so the file pins that behaviour; regenerate it only when the policy is MEANT to
change.

No GPU and no library: the compute object (an "object" scene of four Gaussians on the CPU) is driven with stand-ins for
the three things `_cut_flag` talks to
  * `rz.context(device)`          -> FakeContext: `fenced()` and `cut_retries`
  * the rasterizer workspace      -> FakeWorkspace: `prev_hint_key`, `hint_key`, `cut_block`, `cap`, a CPU `buf`
  * `lib()`                       -> FakeLib: serves `mgr_raster_layout`, records the `mgr_raster_set_cut_*` arguments
and, between two forwards, a stand-in for the device: it overwrites the two hint regions of the workspace with bytes that
name the forward, so that parked and restored tables can be told apart.

The file holds the script (a list of operations) and, per "forward", one record
    [bits `_cut_flag` returned, library calls it made (floats as `float.hex()`: compared bit for bit),
     generation and views it left in `ws.hint_key`, `ws.cut_block`, hint region tile_zcut, hint region tile_zwin]
with the two regions as `_cut_flag` left them (hex).
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

V, N, W, H = 2, 4, 16, 16
T = ((W + 15) // 16) * ((H + 15) // 16)
REGION = 4 * V * T                      # bytes of one hint region
N_SLOTS, ZCUT, ZWIN = 33, 26, 32        # mgr_raster_layout: number of offsets, tile_zcut, tile_zwin
OFFSETS = [64 * i for i in range(N_SLOTS)]
PRODUCED_BY = "dc46d62"


class FakeContext:
    def __init__(self):
        self.cut_retries, self.is_fenced = 0, True

    def fenced(self, sync_check=True):
        return self.is_fenced


class FakeRasterizer:
    def __init__(self):
        self.ctx = FakeContext()

    def context(self, device=None):
        return self.ctx


class FakeWorkspace:
    def __init__(self):
        self.cap = 4096
        self.buf = torch.zeros(64 * (N_SLOTS + 1), dtype=torch.uint8)
        self.hint_key = self.prev_hint_key = None
        self.cut_block = False

    def regions(self):
        return [self.buf[OFFSETS[i]: OFFSETS[i] + REGION] for i in (ZCUT, ZWIN)]


class FakeLib:
    def __init__(self):
        self.calls = []

    def mgr_raster_layout(self, V_, N_, W_, H_, cap, out, n_out):
        assert (V_, N_, W_, H_) == (V, N, W, H)
        for i in range(min(N_SLOTS, n_out)):
            out[i] = OFFSETS[i]
        return N_SLOTS

    def mgr_raster_set_cut_margin(self, rel, entries, rel_box, abs_, interior):
        assert isinstance(entries, int) and isinstance(interior, int)
        self.calls.append(["margin", float(rel).hex(), entries, float(rel_box).hex(), float(abs_).hex(), interior])
        return 0

    def mgr_raster_set_cut_penalty(self, n):
        assert isinstance(n, int)
        self.calls.append(["penalty", n])
        return 0


def script():
    """The operations of the trace.  ["forward", views, flagged, cut_block, fenced]: `flagged` bumps the context's
    `cut_retries` before the launch, `cut_block` sets the workspace's flag (both are what resolving the fence of a flagged
    forward does); ["tick", n]: n parameter updates; ["set_params"]; ["set", attribute, value]: a switch of the object."""
    a, b, c = [0, 1], [2, 3], [4, 5]
    fwd = lambda views, flagged=False, block=False, fenced=True: ["forward", views, flagged, block, fenced]
    ops = []
    # on-device repair (the default): first sight of a view set (no usable hints), clean forwards, another view set and back
    # (park / restore), a third one with room for two parked sets only (the oldest is dropped: zeros on its return)
    ops += [fwd(a, fenced=False), fwd(a), fwd(a), fwd(a), fwd(b), fwd(b), fwd(a), fwd(b), fwd(c), fwd(a), fwd(b), fwd(c), fwd(a)]
    # an unfenced forward in between leaves hints nobody may use
    ops += [fwd(a, fenced=False), fwd(a), fwd(a)]
    # flagged under the repair: the re-run on full lists, a short pause, then the cut again
    ops += [fwd(a, flagged=True, block=True), fwd(a), fwd(a), fwd(a), fwd(a), fwd(a), fwd(a)]
    ops += [["set", "cut_margin", 0.3], ["set", "cut_penalty", 5], fwd(a), fwd(a), ["set", "cut_margin", 1.0], ["set", "cut_penalty", 16]]
    # the parameters move: hints within cut_max_age updates are used, older ones are not
    ops += [["tick", 16], fwd(a), ["tick", 17], fwd(a), fwd(a), ["tick", 3], fwd(b), fwd(b)]
    # more view sets than four times the parked-set limit: the table of hint ages is pruned
    ops += [["tick", 20]] + [fwd([10 + i, 11 + i]) for i in range(10)] + [fwd(a), fwd(a)]
    # densification: a new generation, parked hints dropped
    ops += [fwd(b), ["set_params"], fwd(a), fwd(a), fwd(b), fwd(a)]
    # the cut switched off and on again
    ops += [["set", "depth_cut", False], fwd(a), ["set", "depth_cut", True], fwd(a), fwd(a)]
    # legacy mode (flag, re-run, back-off): clean forwards at the 1x clamp of the margins, one flagged forward and its pause
    ops += [["set", "cut_repair", False], fwd(a), fwd(a), fwd(a, flagged=True, block=True)] + [fwd(a) for _ in range(7)]
    # flagged again and again: the margins double up to 32x, the back-off up to 512 -- the pause that follows is 512 forwards
    # long, during which the margins come down by 2 % per forward to the 1x clamp
    ops += [fwd(a, flagged=True, block=True) for _ in range(10)] + [fwd(a) for _ in range(512 + 3)]
    # 32 clean forwards in a row halve the back-off, 66 in all do it twice: the next flagged forward pauses for 128
    ops += [fwd(a) for _ in range(63)] + [fwd(a, flagged=True, block=True)] + [fwd(a) for _ in range(128 + 2)] + [fwd(b), fwd(a)]
    # the repair mode drains a long pause in four forwards
    ops += [fwd(a, flagged=True, block=True), ["set", "cut_repair", True]] + [fwd(a) for _ in range(6)]
    return ops


def drive(ops):
    """Run the operations on a fresh compute object; the list of records, one per "forward"."""
    from manus_amd import _lib, engine
    fake = FakeLib()
    # (`lib` as the engine finds it: looked up in `_lib` at call time, or bound in the engine module at import)
    patched = [(m, m.lib) for m in (_lib, engine) if hasattr(m, "lib")]
    for m, _ in patched:
        m.lib = lambda: fake
    try:
        params = {k: torch.zeros((N, w)) for k, w in (("_xyz", 3), ("_opacity", 1))}
        c = engine.HipViewCompute(dict(kind="object", params=params), None, None, depth_cut=True, max_cut_hints=2)
        assert c.depth_cut, "MANUS_DEPTH_CUT=0 in the environment"
        c.rz = FakeRasterizer()
        ctx, ws = c.rz.ctx, FakeWorkspace()
        out = []
        for op in ops:
            if op[0] == "tick":
                for _ in range(op[1]):
                    c.mark_params_changed()
            elif op[0] == "set_params":
                c.set_params(params)
            elif op[0] == "set":
                setattr(c, op[1], op[2])
            else:
                _, views, flagged, block, fenced = op
                ctx.cut_retries += int(flagged)
                ws.cut_block = ws.cut_block or block
                ctx.is_fenced = fenced
                ws.prev_hint_key, ws.hint_key = ws.hint_key, None          # (RasterContext.forward, before the launch)
                fake.calls = []
                bits = c._cut_flag(ws, views, V, N, W, H)
                key = ws.hint_key
                out.append([int(bits), fake.calls, None if key is None else [int(key[1])] + list(key[2]), bool(ws.cut_block)]
                           + [bytes(r.tolist()).hex() for r in ws.regions()])
                for j, r in enumerate(ws.regions()):                       # the "device": this forward's hints
                    r.copy_(torch.tensor([(len(out) * 7 + 3 * j + i) % 251 + 1 for i in range(REGION)], dtype=torch.uint8))
        return out
    finally:
        for m, f in patched:
            m.lib = f


def main():
    ops = script()
    rec = drive(ops)
    path = os.path.join(HERE, "depth_cut_policy.json")
    with open(path, "w") as f:
        json.dump(dict(produced_by=PRODUCED_BY, script=ops, forwards=rec), f, separators=(",", ":"))
        f.write("\n")
    seen = sorted({r[0] for r in rec})
    print("%s: %d forwards, bits seen %s, %d bytes" % (path, len(rec), seen, os.path.getsize(path)))


if __name__ == "__main__":
    main()
