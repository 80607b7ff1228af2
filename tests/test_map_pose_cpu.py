"""No GPU: the ABI of the map backward's pose gradient (mgr_views_maps_backward_pose, mgr_views_maps_pose_workspace_bytes) --
header, binding, built library --, the size function against its documented formula, and the refusals that are decided before
anything touches a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"mgr_views_maps_pose_workspace_bytes": 3, "mgr_views_maps_backward_pose": 34, "mgr_skin_rows_mask": 5}
MAX_WG = 1024          # MGR_POSE_MAX_WG (csrc/instance_math.h)


def _declared_args(header, name):
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % re.escape(name), header, re.S)
    assert m, "include/manus_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from manus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "manus_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NEW_ENTRIES.items():
        assert len(_declared_args(header, name)) == arity, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity, (name, len(args))
        assert res is (ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int), name
        assert hasattr(so, name), "%s is not exported by the built library" % name
    # every argument of mgr_views_maps_backward, in its order, then the pose arguments, the stream last
    plain, pose = _declared_args(header, "mgr_views_maps_backward"), _declared_args(header, "mgr_views_maps_backward_pose")
    assert pose[:len(plain) - 1] == plain[:-1] and pose[-1] == plain[-1]
    assert pose[len(plain) - 1:-1] == ["int accumulate_pose", "float* d_transforms", "void* pose_workspace", "size_t pose_workspace_bytes"]
    a, b = _lib.SIGNATURES["mgr_views_maps_backward"][1], _lib.SIGNATURES["mgr_views_maps_backward_pose"][1]
    assert b[:len(a) - 1] == a[:-1] and b[-1] is a[-1]


def _formula(V, N, B):
    if V <= 0 or N <= 0 or B <= 0:
        return 0
    G = 1 if V <= 1 else 2 if V <= 2 else 4 if V <= 4 else 8
    slots = min(MAX_WG, -(-N // (256 // G)))
    return (slots * G * B * 12 * 4 + 255) // 256 * 256


def test_pose_workspace_bytes():
    from manus_amd._lib import lib
    f = lib().mgr_views_maps_pose_workspace_bytes
    for V, N, B in ((0, 10, 21), (-1, 10, 21), (3, 0, 21), (3, -5, 21), (3, 10, 0), (3, 10, -2)):
        assert f(V, N, B) == 0, (V, N, B)
    for V in (1, 2, 3, 4, 5, 8, 9, 11, 64):
        for B in (1, 21, 32):
            prev = 0
            for N in (1, 31, 32, 33, 255, 256, 257, 2000, 32 * MAX_WG - 1, 32 * MAX_WG, 32 * MAX_WG + 1, 256 * MAX_WG, 256 * MAX_WG + 1, 10 ** 7):
                got = f(V, N, B)
                assert got == _formula(V, N, B), (V, N, B, got)
                assert got >= prev > -1, (V, N, B)          # monotone in N ...
                prev = got
            assert prev == _formula(V, 2 ** 31 - 1, B) == f(V, 2 ** 31 - 1, B)      # ... up to the cap
    assert f(8, 300000, 32) == MAX_WG * 8 * 32 * 12 * 4                                # the bound: 12.6 MB
    assert f(8, 2000, 21) == (63 * 8 * 21 * 12 * 4 + 255) // 256 * 256                 # 63 chunks of 32: nothing per (Gaussian, view)


def test_refusals_before_the_device():
    """Every refusal that is decided on the arguments alone: the stated code, mgr_last_error() naming the entry, nothing read
    through the (fake, never dereferenced) pointers."""
    from manus_amd._lib import MGR_EINVAL, MGR_ENOMEM, lib
    L = lib()
    V, N, B, W, H, cap = 3, 100, 21, 56, 40, 4096
    need = int(L.mgr_views_maps_pose_workspace_bytes(V, N, B))
    p = ctypes.c_void_p(0x1000)
    names = ("cams", "xyz", "log_scale", "rot", "opacity_logit", "skin_w", "transforms", "out_alpha", "out_depth", "dL_dalpha", "dL_ddepth",
             "d_xyz", "d_log_scale", "d_rot", "d_opacity_logit", "d_skin_w", "workspace", "scratch", "d_transforms", "pose_workspace")

    def call(B=B, na=N, pose_bytes=need, **null):
        a = {k: (None if null.get(k) else p) for k in names}
        assert set(null) <= set(names)
        return L.mgr_views_maps_backward_pose(V, N, B, na, W, H, a["cams"], a["xyz"], a["log_scale"], a["rot"], a["opacity_logit"], a["skin_w"],
                                              a["transforms"], a["out_alpha"], a["out_depth"], a["dL_dalpha"], a["dL_ddepth"], 0, a["d_xyz"],
                                              a["d_log_scale"], a["d_rot"], a["d_opacity_logit"], a["d_skin_w"], a["workspace"], 1 << 40, cap,
                                              a["scratch"], 1 << 40, 0, 0, a["d_transforms"], a["pose_workspace"], pose_bytes, None)

    def refused(rc, code, text=None):
        err = L.mgr_last_error()
        assert rc == code, (rc, code, err)
        assert b"mgr_views_maps_backward_pose" in err, err
        if text:
            assert text in err, err

    for k in ("cams", "xyz", "rot", "transforms", "d_xyz", "d_skin_w", "workspace", "scratch", "out_alpha"):
        refused(call(**{k: True}), MGR_EINVAL, b"null pointer")
    refused(call(dL_dalpha=True, dL_ddepth=True), MGR_EINVAL, b"both NULL")
    refused(call(skin_w=True), MGR_EINVAL, b"skin_w")
    refused(call(d_transforms=True), MGR_EINVAL, b"d_transforms")
    refused(call(pose_workspace=True), MGR_EINVAL, b"pose_workspace")
    for bad_B in (0, -1, 33):
        refused(call(B=bad_B), MGR_EINVAL, b"bad B")
    for bad_na in (0, -3):
        refused(call(na=bad_na), MGR_EINVAL)
    refused(call(na=N + 1), MGR_EINVAL, b"n_articulated")
    refused(call(pose_bytes=need - 1), MGR_ENOMEM, b"pose workspace")
    refused(call(pose_bytes=0), MGR_ENOMEM, b"pose workspace")
    # the plain entry keeps its name in its own refusals
    rc = L.mgr_views_maps_backward(V, N, B, N, W, H, p, p, p, p, p, p, p, None, None, None, None, 0, p, p, p, p, p, p, 1 << 40, cap, p, 1 << 40, 0, None)
    assert rc == MGR_EINVAL and b"mgr_views_maps_backward:" in L.mgr_last_error()


def test_rows_mask_refusals_before_the_device():
    """mgr_skin_rows_mask (the row mask behind the fused step's non-zero-row list): refusals on the arguments alone; n = 0 is a
    no-op that needs no pointer."""
    from manus_amd._lib import MGR_EINVAL, lib
    L = lib()
    p = ctypes.c_void_p(0x1000)
    for args in ((-1, 21, p, p), (10, 0, p, p), (10, 33, p, p), (10, 21, None, p), (10, 21, p, None)):
        assert L.mgr_skin_rows_mask(*args, None) == MGR_EINVAL, args
        assert b"mgr_skin_rows_mask" in L.mgr_last_error()
    assert L.mgr_skin_rows_mask(0, 21, None, None, None) == 0
