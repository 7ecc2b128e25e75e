"""CPU-side checks of the path resampling boundary (dcx_path_resample, dcx_path_resample_work_bytes): the symbols exist and the
version stays 109, the header and the ctypes table declare the same arguments, the header section is marked as added under
version 109 and states the contract's load-bearing words, every argument error is reported before anything touches a device,
the workspace size is 0 for refused arguments and monotone, and the Python layer refuses its mistakes - on a machine without a
GPU."""
import ctypes

import pytest

from test_rrt_abi import HEADER, _declared

NAMES = ["dcx_path_resample", "dcx_path_resample_work_bytes"]


@pytest.mark.parametrize("name", NAMES)
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("batched path resampling")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    body = src[at:][:9000]
    for word in ("fixed association", "largest index", "is not written", "non-decreasing", "#define DCX_RESAMPLE_CHUNK 32"):
        assert word in body, word
    assert "#define DCX_VERSION 109" in src


def _run(lib, R=8, W=32, dof=3, mask=0, T=16, path=1, count=1, out=1, out_count=1, length=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    return lib.dcx_path_resample(0, p(path), p(count), R, W, dof, mask, T, p(out), p(out_count), p(length), p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    need = lib.dcx_path_resample_work_bytes(8, 4096)
    assert need >= 2 * 8 * 4096 * 4
    cases = [
        (dict(R=-1), "R < 0"),
        (dict(W=0), "W must be in [1, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(W=65537), "W must be in [1, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(T=1), "T must be in [2, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(T=0), "T must be in [2, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(T=-3), "T must be in [2, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(T=65537), "T must be in [2, DCX_SHORTCUT_MAX_WAYPOINTS]"),
        (dict(dof=0), "dof < 1"),
        (dict(dof=-2), "dof < 1"),
        (dict(mask=0b1000), "wrap_mask has a bit at or above dof"),
        (dict(mask=1 << 63), "wrap_mask has a bit at or above dof"),
        (dict(path=0), "path or count is NULL"),
        (dict(count=0), "path or count is NULL"),
        (dict(out=0), "out or out_count is NULL"),
        (dict(out_count=0), "out or out_count is NULL"),
        (dict(work=0), "work is NULL"),
        (dict(W=4096, work_bytes=need - 1), "smaller than dcx_path_resample_work_bytes"),
        (dict(work_bytes=0), "smaller than dcx_path_resample_work_bytes"),
    ]
    for kw, text in cases:
        rc = _run(lib, **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # beyond one launch and beyond the compiled dof: unsupported, not invalid
    assert _run(lib, R=1 << 31, work_bytes=1 << 62) == 2
    assert "2^31 - 1" in lib.dcx_last_error().decode()
    assert _run(lib, dof=33) == 2
    assert "DCX_MAX_DOF" in lib.dcx_last_error().decode()
    # nothing to do is not an error, with or without buffers; the limits themselves are accepted
    assert _run(lib, R=0, path=0, count=0, out=0, out_count=0, length=0, work=0, work_bytes=0) == 0
    assert _run(lib, R=0, W=65536, T=65536, dof=32, mask=(1 << 32) - 1) == 0
    assert _run(lib, R=0, T=2, W=1) == 0


def test_work_bytes_is_zero_for_refused_arguments_and_monotone():
    from diffco_amd import _lib
    wb = _lib.load().dcx_path_resample_work_bytes
    for bad in [(-1, 32), (8, 0), (8, -1), (8, 65537), (1 << 31, 32)]:
        assert wb(*bad) == 0, bad
    for W in (1, 31, 32, 33, 2048, 2049, 65536):
        sizes = [wb(R, W) for R in (0, 1, 7, 64, 1000, 1 << 20, (1 << 31) - 1)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > 0, (W, sizes)
    for R in (0, 1, 67, 1 << 20):
        sizes = [wb(R, W) for W in (1, 2, 31, 32, 33, 1024, 2048, 2049, 4096, 65535, 65536)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (R, sizes)
    # a row too long for a block's LDS keeps its arc lengths and segment lengths in the workspace
    assert wb(67, 65536) >= 2 * 67 * 65536 * 4


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import resample, resample_paths
    assert resample.resample_paths is resample_paths
    p = [torch.zeros(4, 3)]
    with pytest.raises(ValueError, match="n_waypoints"):
        resample_paths(p, n_waypoints=1)
    with pytest.raises(ValueError, match="bit at or above dof"):
        resample_paths(p, n_waypoints=4, wrap=0b1000)
    with pytest.raises(ValueError, match="come with `counts`"):
        resample_paths(torch.zeros(2, 4, 3), n_waypoints=4)
    # shortcut_paths' other mistakes, refused alike
    with pytest.raises(ValueError, match="counts must be 2 integers"):
        resample_paths(torch.zeros(2, 4, 3), torch.tensor([1, 5]), n_waypoints=4)
    with pytest.raises(ValueError, match="`counts` goes with a tensor"):
        resample_paths(p, torch.tensor([4]), n_waypoints=4)
    with pytest.raises(ValueError, match="same dof"):
        resample_paths([torch.zeros(4, 3), torch.zeros(4, 2)], n_waypoints=4)
    with pytest.raises(ValueError, match="at least one path"):
        resample_paths([None], n_waypoints=4)
    with pytest.raises(ValueError, match="wrap=True needs a transform"):
        resample_paths(p, n_waypoints=4, wrap=True)
