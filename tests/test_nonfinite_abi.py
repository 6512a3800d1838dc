"""The checked forward entry points (include/mdc.h, "non-finite input frames"): declared, bound, exported by both libraries,
usable from C99, and validating their arguments before any device call (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from modulationdetectioncnn_amd import _cabi

NEW = ("mdc_forward_checked", "mdc_predict_host_checked")


def _declared():
    text = open(os.path.join(ROOT, "include", "mdc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mdc_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_declare_the_checked_entries():
    for name in NEW:
        assert name in _declared() and name in _cabi.EXPORTS
    assert sorted(_cabi.EXPORTS) == _declared()
    assert (_cabi.NONFINITE_REPORT, _cabi.NONFINITE_PROPAGATE) == (0, 1)
    assert _cabi.ABI_VERSION == 5


def test_both_libraries_export_the_checked_entries():
    import modulationdetectioncnn_amd.build as b
    for variant in b.VARIANTS:
        out = subprocess.run(["nm", "-D", "--defined-only", b.build(variant=variant)], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for name in NEW:
            assert name in names, (variant, name)


def test_header_policies_compile_as_c99(tmp_path):
    src = tmp_path / "nf.c"
    src.write_text('#include "mdc.h"\n'
                   'static int (*fwd)(const mdc_model*, const void*, int64_t, float*, int32_t*, void*, size_t, uint8_t*, int64_t*, int, void*)'
                   ' = mdc_forward_checked;\n'
                   'static int (*host)(mdc_model*, const float*, int64_t, float*, int32_t*, uint8_t*, int64_t*, int, int64_t)'
                   ' = mdc_predict_host_checked;\n'
                   'int main(void) { return (fwd && host && MDC_NONFINITE_REPORT == 0 && MDC_NONFINITE_PROPAGATE == 1) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


@pytest.mark.parametrize("variant", ["product", "alternates"])
def test_checked_entries_validate_their_arguments_without_gpu(variant):
    L = _cabi.lib(variant)
    err = lambda: L.mdc_last_error()      # noqa: E731
    buf = (ctypes.c_uint8 * 2048)()
    base = (ctypes.addressof(buf) + 15) & ~15            # 16-byte aligned host memory: every check below comes before a launch
    flags = ctypes.addressof(buf) + 1536
    fwd = L.mdc_forward_checked
    assert fwd(None, base, 1, None, None, None, 0, flags, None, 0, None) == -22 and b"null model" in err()
    assert fwd(None, base, 1, None, None, None, 0, None, None, 0, None) == -22 and b"nonfinite_dev" in err()
    assert fwd(None, base, 1, None, None, None, 0, flags, None, 2, None) == -22 and b"policy" in err()
    assert fwd(None, base, 1, None, None, None, 0, flags, None, -1, None) == -22 and b"policy" in err()
    assert fwd(None, base, -1, None, None, None, 0, flags, None, 1, None) == -22 and b"negative" in err()
    assert fwd(None, base + 4, 1, None, None, None, 0, flags, None, 1, None) == -22 and b"aligned" in err()
    assert fwd(None, None, 1, None, None, None, 0, flags, None, 1, None) == -22 and b"null input" in err()
    host = L.mdc_predict_host_checked
    assert host(None, base, 4, None, None, flags, None, 0, 0) == -22 and b"null model" in err()
    assert host(None, base, 4, None, None, None, None, 0, 0) == -22 and b"nonfinite_host" in err()
    assert host(None, base, 4, None, None, flags, None, 7, 0) == -22 and b"policy" in err()
    assert host(None, base, -4, None, None, flags, None, 0, 0) == -22


def test_python_surface_refuses_bad_nonfinite_arguments_without_gpu():
    from modulationdetectioncnn_amd import NonFiniteInputError, Topology, VTCNN2
    from modulationdetectioncnn_amd.model import _nonfinite_policy
    assert issubclass(NonFiniteInputError, ValueError)
    e = NonFiniteInputError([3, 17])
    assert e.frames == [3, 17] and e.count == 2 and "3, 17" in str(e)
    assert _nonfinite_policy(None) is None
    assert _nonfinite_policy("propagate") == _cabi.NONFINITE_PROPAGATE and _nonfinite_policy("raise") == _cabi.NONFINITE_REPORT
    with pytest.raises(ValueError, match="nonfinite"):
        _nonfinite_policy("ignore")
    with pytest.raises(ValueError, match="tap"):
        _nonfinite_policy("propagate", "dense")
    m = VTCNN2(Topology.deployed(3, 3), device=None)
    import numpy as np
    x = np.zeros((2, 2, 128), np.float32)
    with pytest.raises(ValueError, match="tap"):
        m.predict(x, tap="dense", nonfinite="raise")          # refused before the model would need a device
    with pytest.raises(ValueError, match="nonfinite"):
        m.predict_host(x, nonfinite="nan")
