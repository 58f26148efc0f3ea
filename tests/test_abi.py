"""The C-ABI library loads and exports every symbol include/sqe.h declares (no compute
calls: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "sqe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sqe_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "semantic_query_engine_amd", "libsqe.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from semantic_query_engine_amd import _native
    return _native.load()


def test_header_symbols_are_exported_and_bound(lib):
    from semantic_query_engine_amd import _native
    declared = _declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in sqe.h but not exported"
    assert sorted(_native.SIGNATURES) == declared      # the ctypes table covers the header exactly


def test_version_and_error_string(lib):
    assert lib.sqe_version() == 100
    assert isinstance(lib.sqe_last_error(), bytes)


def test_struct_layouts_match_header():
    from semantic_query_engine_amd import _native
    assert ctypes.sizeof(_native.BertCfg) == 32
    assert ctypes.sizeof(_native.EncoderState) == 8 * 4 + 8 + 4 * 12            # sqe_encoder_state_t
    assert ctypes.sizeof(_native.IvfSearchState) == 3 * 8 + 22 * 4                # sqe_ivf_state_t
    assert ctypes.sizeof(_native.ScanLaunch) == 8 + 22 * 4                        # sqe_scan_launch_t
    assert ctypes.sizeof(_native.I8Launch) == 88                                  # sqe_i8_launch_t: 2 x 8 + 18 x 4
    assert ctypes.sizeof(_native.DeleteLast) == 9 * 8                             # sqe_delete_last_t
    assert ctypes.sizeof(_native.Stats) == 6 * 8 + 6 * 8 + 4 * 8      # + sample_ms and the three int8 counters (r03)


def test_i8_read_constants_match_header():
    """engine.I8_* are the values of the header's SQE_I8_* buffer enum (sqe_index_i8_read), the select read-backs included."""
    from semantic_query_engine_amd import engine as E
    text = open(os.path.join(ROOT, "include", "sqe.h")).read()
    body = re.search(r"enum \{ (SQE_I8_ROWS = 0.*?) \};", text, flags=re.S).group(1)
    header = {name: int(val) for name, val in re.findall(r"SQE_(I8_[A-Z_0-9]+) = (\d+)", body)}
    assert len(header) == 17 and sorted(header.values()) == list(range(17))
    for name in ("I8_THR_EFF", "I8_SAMPLE_COS", "I8_SAMPLE_IDS", "I8_SELECT_COS", "I8_SELECT_IDS", "I8_SELECT_THR", "I8_SELECT_TRACE"):
        assert name in header
    for name, val in header.items():
        assert getattr(E, name) == val, name


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import importlib
    from semantic_query_engine_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        _native.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "semantic_query_engine_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), encoding="utf-8").read()
                assert "oracle" not in text.replace("no CPU fallback", ""), f"{f} mentions the oracle"
