"""CPU checks of the material maps (nmf_material_maps, renderer.map_to_8bit, the --material-maps flags): the entry point is exported and
refuses bad arguments without a GPU, the 8-bit conversion is the reference's truncation with a clip, and the flags need their
evaluation flag."""
import ctypes as C

import numpy as np
import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    return hip, lib


def _call(lib, B=4, M=10, Mb=2, R=5, ptr=C.c_void_p(16), rows=None, app=None):
    one = ptr
    rows = one if rows is None else rows
    app = one if app is None else app
    f = C.c_float(0.0)
    return lib.nmf_material_maps(app, one, one, one, C.c_int64(B), C.c_int64(M), one, one, one, f, f, f, f, f, one,
                                 rows, rows, rows, C.c_int64(Mb), rows, rows, C.c_int64(R), one, one, one, None)


def test_material_maps_is_exported_and_checks_its_arguments():
    hip, lib = _lib()
    assert "nmf_material_maps" in hip.EXPORTS and hasattr(lib, "nmf_material_maps")
    assert hip.version() >= 118
    # (the pointers are never dereferenced: every call below fails on its arguments or has nothing to do)
    assert _call(lib, B=-1) == -1 and b"nmf_material_maps" in lib.nmf_last_error_string()
    assert _call(lib, M=-3) == -1 and _call(lib, Mb=-1, R=0) == -1 and _call(lib, R=-2) == -1
    assert _call(lib, Mb=3, R=2) == -1                       # every bounce row has at least one secondary ray
    assert _call(lib, M=1, Mb=2) == -1                       # more rows than samples
    assert _call(lib, Mb=0, R=4) == -1                       # secondary rays without rows
    assert _call(lib, ptr=None) == -1 and b"null" in lib.nmf_last_error_string()
    assert _call(lib, app=C.c_void_p(0)) == -1 and b"sample input" in lib.nmf_last_error_string()
    assert _call(lib, rows=C.c_void_p(0)) == -1 and b"row input" in lib.nmf_last_error_string()
    assert _call(lib, B=0, ptr=None, rows=None) == 0         # no ray: nothing to do


def test_material_maps_wrapper_refuses_cpu_tensors():
    hip, _ = _lib()
    z = lambda *s: torch.zeros(*s)                            # noqa: E731
    with pytest.raises(hip.NmfHipError):
        hip.material_maps(z(4, 24), z(4, 3), z(4), torch.tensor([0, 4], dtype=torch.int64), z(1, 6), z(11, 24), z(11),
                          (1.0, 0.0, 0.0, 0.0, 0.0), z(9, 3), z(1), z(3))
    with pytest.raises(hip.NmfHipError):
        hip.material_maps(z(4, 24), z(4, 3), z(4), torch.tensor([0, 4], dtype=torch.int64), z(1, 6), z(11, 24), z(11),
                          (1.0, 0.0), z(9, 3), z(1), z(3))


def test_map_to_8bit_truncates_like_the_reference_and_clips():
    from nmf_amd.renderer import map_to_8bit
    x = np.array([[0.0, 0.5, 1.0], [0.999, 0.00393, 0.0039]], dtype=np.float32)
    ref = (x * 255).astype(np.uint8)                                 # renderer.py:440-463 inside [0, 1]
    assert np.array_equal(map_to_8bit(x), ref) and map_to_8bit(x).dtype == np.uint8
    assert map_to_8bit(x).tolist() == [[0, 127, 255], [254, 1, 0]]
    y = np.array([-0.2, 1.7, 3.0, np.float32(256 / 255)], dtype=np.float32)
    assert map_to_8bit(y).tolist() == [0, 255, 255, 255]              # astype(uint8) alone would wrap 1.7 * 255 to 177
    assert map_to_8bit(np.zeros((2, 3, 3))).shape == (2, 3, 3)


def test_material_maps_flag_needs_its_evaluation_flag(capsys):
    from nmf_amd import render as R
    from nmf_amd import train as T
    with pytest.raises(SystemExit):
        R.main(["--ckpt", "missing.th", "--material-maps"])
    assert "--material-maps needs --eval-dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.main(["--iters", "1", "--material-maps"])
    assert "--material-maps needs --render-test" in capsys.readouterr().err
