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


def _listed_values(desc):
    """the values a knob's description names: "N = meaning", "a | b | c" lists and "(0 fp32 MFMA, 1 bf16 split, ...)" enumerations;
    "<= 0 = default" is a setter normalisation, not an arm"""
    desc = re.sub(r"[<>]=?\s*-?\d+\s*=", "", desc)
    vals = {int(v) for v in re.findall(r"(?<![\w.*])(-?\d+) =", desc)}
    for lst in re.findall(r"-?\d+(?: \| -?\d+)+", desc):
        vals |= {int(v) for v in lst.split(" | ")}
    for lst in re.findall(r"\((\d+ [a-z][^()]*)\)", desc):
        items = [re.match(r"(\d+) [a-zA-Z]", it.strip()) for it in lst.split(",")]
        if len(items) > 1 and all(items):
            vals |= {int(m.group(1)) for m in items}
    return vals


def test_every_knob_arm_has_a_test():
    """Every ordinary knob of the registry is in tests/test_arms_gpu.py ARMS — with an entry for each non-default value its description
    names — or in COVERED_BY, pointing at an existing test function whose source sets it; only the wrong-result switches of the ablation
    builds are exempt.  A knob added without a test fails here, by name."""
    import inspect
    import importlib
    from dcnet_amd.lib import tuning as read
    import test_arms_gpu as A
    knobs = read()
    assert set(A.ARMS) | set(A.COVERED_BY) | set(A.EXEMPT) <= set(knobs), "the tables name knobs the registry does not have"
    for knob, (which, flag) in A.EXEMPT.items():
        assert flag.startswith("-D") and which, knob
        assert knobs[knob]["ablation"] == 1 or knob in A.ARMS or knob in A.COVERED_BY, f"{knob}: only its wrong-result values are exempt"
    missing = [k for k, v in knobs.items() if v["ablation"] == 0 and k not in A.ARMS and k not in A.COVERED_BY]
    assert not missing, f"knobs without a test of their arms: {missing} (tests/test_arms_gpu.py ARMS / COVERED_BY)"
    for knob, v in knobs.items():
        if v["ablation"] != 0 and knob not in A.ARMS and knob not in A.COVERED_BY:
            assert knob in A.EXEMPT, f"{knob}: an ablation-only switch must be listed in EXEMPT with its compile flag"
    for knob, arms in A.ARMS.items():
        assert arms, knob
        set_to = set()
        for values, workload, evidence in arms:
            assert knob in values and workload[0] in A.WORKLOADS and evidence[0], (knob, values)
            set_to.add(values[knob])
        want = _listed_values(knobs[knob]["desc"]) - {knobs[knob]["default"]}
        assert want <= set_to, f"{knob}: no ARMS entry for the value(s) {sorted(want - set_to)} its description lists"
        assert set_to - {knobs[knob]["default"]}, f"{knob}: no entry sets it to anything but its default"
    for knob, where in A.COVERED_BY.items():
        mod = importlib.import_module(where[0])
        fn = getattr(mod, where[1], None)
        assert callable(fn) and where[1].startswith("test_"), f"{knob}: {where[0]}.{where[1]} is not a test function"
        src = inspect.getsource(fn)
        if len(where) > 2:
            assert where[2] + "(" in src, f"{knob}: {where[1]} does not call {where[2]}"
            src = inspect.getsource(getattr(mod, where[2]))
        assert f'"{knob}"' in src, f"{knob}: the source of {'.'.join(where)} does not mention it"
    # no case of the arm tests may be skipped or expected to fail
    src = inspect.getsource(A)
    for banned in ("pytest.skip", "mark.skip", "skipif", "xfail", "importorskip"):
        assert banned not in src, f"tests/test_arms_gpu.py uses {banned}"


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
