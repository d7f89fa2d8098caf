"""CPU: the knob registry behind dcn_set_tuning (csrc/tuning.h) — exact names, readable values, wrong-result switches refused by a
default build — and the build stamp of dcnet_amd/build.py.  dcn_set_tuning is host code: no device needed."""
import os
import re
import stat

import pytest

from util import ROOT, tuning


def test_every_knob_round_trips_and_the_readme_table_lists_them_all():
    from dcnet_amd.lib import lib, tuning as read
    names, L = [], lib()._dll
    import ctypes
    name = ctypes.c_char_p()
    while L.dcn_tuning_info(len(names), ctypes.byref(name), None, None, None, None) == 0:
        names.append(name.value.decode())
    assert "past the last knob" in L.dcn_last_error().decode()
    assert len(names) >= 40 and len(set(names)) == len(names)
    knobs = read()
    assert list(knobs) == names
    with tuning():
        for k, v in knobs.items():
            lib().set_tuning(k.encode(), v["default"])
            assert read()[k]["value"] == v["default"], k
            assert v["desc"] and v["ablation"] in (0, 1, 2)
    text = open(os.path.join(ROOT, "README.md")).read()
    table = text[text.index("<!-- knobs -->"):text.index("<!-- /knobs -->")]
    rows = re.findall(r"^\| `([^`]+)` \| (-?\d+) \|", table, flags=re.M)
    assert sorted(n for n, _ in rows) == sorted(names)
    assert {n: int(d) for n, d in rows} == {k: v["default"] for k, v in knobs.items()}


@pytest.mark.parametrize("key", ["wide", "bpc", "precison", "1", "3x3", "9targ", "quiet", "", "Precision", "precision "])
def test_keys_are_matched_whole(key):
    from dcnet_amd.lib import DcnError, lib, tuning as read
    before = read()
    with pytest.raises(DcnError) as e:
        lib().set_tuning(key.encode(), 1)
    assert f'"{key}"' in str(e.value)
    assert read() == before


def test_default_build_refuses_wrong_result_switches():
    from dcnet_amd.lib import DcnError, ablation_build, lib, tuning as read
    if ablation_build():
        pytest.fail("the library in the tree is an ablation build (-DDCN_ABL=1): rebuild the default")
    with tuning():
        for key, bad, flag in (("abl", 1, "-DDCN_ABL=1"), ("3abl", 1, "-DC3_ABL=1"), ("Slabfold", -1, "-DDCN_ABL=1"), ("Gemm3", 17, "-DG3_ABL=1")):
            before = read()[key]["value"]
            with pytest.raises(DcnError) as e:
                lib().set_tuning(key.encode(), bad)
            assert flag in str(e.value) and key in str(e.value)
            assert read()[key]["value"] == before
        for key, ok in (("abl", 0), ("3abl", 0), ("Slabfold", 0), ("Slabfold", 4096), ("Gemm3", 257), ("Gemm3", 1)):
            lib().set_tuning(key.encode(), ok)
            assert read()[key]["value"] == ok
        assert read()["abl"]["ablation"] == 1 and read()["3abl"]["ablation"] == 1 and read()["Gemm3"]["ablation"] == 0


def test_setter_normalisations_are_the_declared_ones():
    from dcnet_amd.lib import lib, tuning as read
    with tuning():
        for key in ("9target", "v3target", "xwgtarget", "zwgsmall", "qtargetb16", "qsmallb16"):
            lib().set_tuning(key.encode(), 100)
            assert read()[key]["value"] == 100
            lib().set_tuning(key.encode(), 0)
            assert read()[key]["value"] == read()[key]["default"]
        for p, w in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 4)):
            lib().set_tuning(b"precision", p)
            assert (read()["precision"]["value"], read()["wsplit"]["value"]) == (p, w)
        lib().set_tuning(b"wsplit", 1)
        assert read()["precision"]["value"] == 4
    assert all(v["value"] == v["default"] for v in read().values())


def test_step_ablation_needs_an_ablation_build():
    from dcnet_amd import ops
    assert ops.STEP_ABL == 0
    try:
        ops.STEP_ABL = 1
        with pytest.raises(RuntimeError, match="DCN_ABL"):
            ops._step_abl(1)
    finally:
        ops.STEP_ABL = 0


def test_a_failed_build_does_not_keep_the_default_stamp(tmp_path, monkeypatch):
    """A compile that fails (or is interrupted) must leave build/FLAGS.stamp saying so: the objects under it belong to no finished build."""
    import dcnet_amd.build as b
    objdir = tmp_path / "obj"
    objdir.mkdir()
    (objdir / "FLAGS.stamp").write_text(b.flags_key() + "\n")          # as a finished default build leaves it
    assert b.built_flags_key(str(objdir)) == b.flags_key()
    stub = tmp_path / "hipcc"
    stub.write_text("#!/bin/sh\necho stub compiler fails >&2\nexit 1\n")
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("HIPCC", str(stub))
    lib_before = os.stat(b.OUT).st_mtime_ns if os.path.exists(b.OUT) else None
    with pytest.raises(RuntimeError, match="hipcc failed"):
        b.build(force=True, verbose=False, objdir=str(objdir))
    assert b.built_flags_key(str(objdir)) not in ("", b.flags_key())
    assert (os.stat(b.OUT).st_mtime_ns if os.path.exists(b.OUT) else None) == lib_before
