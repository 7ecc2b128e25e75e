"""CPU-side checks of the wrapped motion calls' boundary (dcx_check_motions_ex, dcx_motion_cost_ex): the header and the ctypes
table declare the same arguments, a wrap mask with a bit at or above dof and every argument error of the plain calls are
reported before anything touches a device, the version stays 109, and the Python layers turn their `wrap` argument into the
mask the C call takes - on a machine without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def _declared(name):
    """(restype, argtypes) of a function as include/dcx.h declares it: every pointer travels as an address"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "*" in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPE[a.replace("const ", "").split()[0]])
    return _CTYPE[m.group(1)], args


@pytest.mark.parametrize("name", ["dcx_check_motions_ex", "dcx_motion_cost_ex", "dcx_check_motions", "dcx_motion_cost"])
def test_header_and_ctypes_signatures_agree(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_ex_takes_the_plain_arguments_plus_the_mask_before_the_stream():
    from diffco_amd import _lib
    for plain in ("dcx_check_motions", "dcx_motion_cost"):
        a, b = list(_lib.SYMBOLS[plain][1]), list(_lib.SYMBOLS[plain + "_ex"][1])
        assert b == a[:-1] + [ctypes.c_uint64] + a[-1:]
    src = open(HEADER).read()
    assert "added under DCX_VERSION 109" in src[src.index("shortest arc of circular coordinates") - 40:][:200]
    # the opts structs keep their layout (their own tests pin the offsets): no new field carries the mask
    assert ctypes.sizeof(_lib.MotionOpts) == 16 and ctypes.sizeof(_lib.MotionCostOpts) == 32


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _check(lib, model, mask=0, E=4, opt=None, qa=1, qb=1, first=1, work=1, work_bytes=1 << 30):
    from diffco_amd._lib import MotionOpts
    opt = MotionOpts(8, 0.0, 8, 0) if opt is None else opt
    p = ctypes.c_void_p
    return lib.dcx_check_motions_ex(model, p(qa), p(qb), E, ctypes.byref(opt) if opt is not False else None, None, p(first), None,
                                    p(work), work_bytes, mask, None)


def _cost(lib, model, mask=0, E=4, opt=None, qa=1, qb=1, cost=1, ga=1, gb=1, work=1, work_bytes=1 << 30):
    from diffco_amd._lib import MotionCostOpts
    opt = MotionCostOpts(8, 0.0, 8, 0) if opt is None else opt
    p = ctypes.c_void_p
    return lib.dcx_motion_cost_ex(model, p(qa), p(qb), E, ctypes.byref(opt) if opt is not False else None, None, 1.0, p(cost),
                                  p(ga), p(gb), None, p(work), work_bytes, mask, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._lib import MotionCostOpts, MotionOpts
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_motion_work_bytes(m, 4)
    need_c = lib.dcx_motion_cost_work_bytes(m, 4, 8)
    both = [
        (dict(mask=1), "wrap_mask has a bit at or above dof"),
        (dict(mask=1 << 63), "wrap_mask has a bit at or above dof"),
        (dict(model=None), "model is NULL"),
        (dict(model=None, mask=1), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(E=-1), "E < 0"),
        (dict(qa=0), "NULL"),
        (dict(qb=0), "NULL"),
        (dict(work=0), "NULL"),
    ]
    check = both + [
        (dict(first=0), "NULL"),
        (dict(opt=MotionOpts(8, 0.5, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(0, 0.0, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(8, 0.0, 0, 0)), "max_samples >= 1"),
        (dict(work_bytes=need - 1), "smaller than dcx_motion_work_bytes"),
    ]
    cost = both + [
        (dict(cost=0), "NULL"),
        (dict(ga=0), "NULL"),
        (dict(gb=0), "NULL"),
        (dict(opt=MotionCostOpts(8, 0.5, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionCostOpts(0, 0.1, 0, 0)), "max_samples >= 1"),
        (dict(opt=MotionCostOpts(0, 0.1, 8, 2)), "open_end must be 0 or 1"),
        (dict(work_bytes=need_c - 1), "smaller than dcx_motion_cost_work_bytes"),
    ]
    for call, cases in ((_check, check), (_cost, cost)):
        for kw, text in cases:
            kw = dict(kw)
            rc = call(lib, kw.pop("model", m), **kw)
            msg = lib.dcx_last_error().decode()
            assert rc == 1, (call.__name__, kw, rc, msg)
            assert text in msg, (call.__name__, kw, msg)
        # nothing to do is not an error, with or without buffers
        assert call(lib, m, E=0, qa=0, qb=0, work=0, work_bytes=0) == 0


class _Owner:
    pass


def test_wrap_argument_becomes_a_mask():
    from diffco_amd._ops import wrap_mask
    assert wrap_mask(None, 7) == 0 and wrap_mask(False, 7) == 0 and wrap_mask(0, 7) == 0
    assert wrap_mask(0b0100101, 7) == 0b0100101
    assert wrap_mask([True, False, True], 3) == 0b101
    assert wrap_mask(torch.tensor([False, False, True]), 3) == 0b100
    assert wrap_mask((1, 1), 2) == 3
    for bad in (1 << 7, -1):
        with pytest.raises(ValueError, match="at or above dof"):
            wrap_mask(bad, 7)
    with pytest.raises(ValueError, match="one bool per coordinate"):
        wrap_mask([True, False], 3)
    with pytest.raises(ValueError, match="one bool per coordinate"):
        wrap_mask([0.5, 0.0, 1.0], 3)
    # True: the mask of the robot whose fkine the transform is - and nothing else
    with pytest.raises(ValueError, match="wrap=True"):
        wrap_mask(True, 3)
    with pytest.raises(ValueError, match="wrap=True"):
        wrap_mask(True, 3, lambda q: q)
    with pytest.raises(ValueError, match="wrap=True"):
        wrap_mask(True, 3, _Owner().__init__)   # a bound method of an object without a wrap_mask


def test_wrap_true_on_the_model_classes():
    from diffco_amd import model
    from diffco_amd._ops import wrap_mask
    from helpers import make_robot
    planar = model.RevolutePlanarRobot([1.0, 0.5, 0.25], 0.1)
    assert planar.wrap_mask == 0b111 and wrap_mask(True, 3, planar.fkine) == 0b111
    assert make_robot("planar7").wrap_mask == 127
    se2 = make_robot("se2")
    assert se2.wrap_mask == 0b100 and wrap_mask(True, 3, se2.fkine) == 0b100
    se3 = make_robot("se3")
    assert se3.wrap_mask == 0b111000 and wrap_mask(True, 6, se3.fkine) == 0b111000
    for name in ("baxter_left", "baxter_right", "baxter_dual", "panda", "panda5", "dual_panda"):
        rob = make_robot(name)
        assert rob.wrap_mask == 0 and wrap_mask(True, rob.dof, rob.fkine) == 0
    # the masks are the coordinates each class's wrap() changes
    for rob in (planar, se2, se3):
        q = torch.full((1, rob.dof), 4.0)
        changed = (rob.wrap(q) != q).reshape(-1).tolist()
        assert sum(1 << j for j, c in enumerate(changed) if c) == rob.wrap_mask


from motion_wrap_helpers import WHEEL_ARM_URDF as _URDF  # noqa: E402


def test_wrap_true_on_urdf_robots_is_their_continuous_joints():
    from diffco_amd._ops import wrap_mask
    from diffco_amd.urdf import MultiURDFRobotFK, URDFRobotFK
    from helpers import urdf_robot
    rob = URDFRobotFK(_URDF)
    assert rob.joint_names == ["yaw", "shoulder", "extend", "spin"]
    assert rob.wrap_mask == 0b1001 and wrap_mask(True, 4, rob.fkine) == 0b1001
    assert torch.equal(rob.wrap(torch.full((1, 4), 4.0)), torch.full((1, 4), 4.0))   # URDFRobotFK.wrap stays the identity
    two = MultiURDFRobotFK([URDFRobotFK(_URDF, name="a"), URDFRobotFK(_URDF, name="b")])
    assert two.wrap_mask == 0b10011001
    assert urdf_robot("urdf_panda").wrap_mask == 0   # revolute joints with limits only


def test_facades_reject_wrap_true_without_an_owner():
    from diffco_amd._perceptron import MotionSource, check_motions, motion_cost, path_cost
    for fn in (check_motions, motion_cost):
        with pytest.raises(ValueError, match="wrap=True"):
            fn(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], res=4, wrap=True)
        with pytest.raises(ValueError, match="at or above dof"):
            fn(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], res=4, wrap=4)
    with pytest.raises(ValueError, match="wrap=True"):
        path_cost(MotionSource(_Owner(), None, lambda q: q, None, None, None), torch.zeros(1, 3, 2), 0.1, wrap=True)
