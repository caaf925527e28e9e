"""tests/family_bounds.py and the seven committed bounds files, on the CPU: the stored numbers follow the rule, the look-up
gives what each family's test computed before the helper existed, a key without an entry is refused, every error figure on
arrays small enough to work out by hand, recording and regenerating."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import family_bounds as FB  # noqa: E402

NAMES = sorted(FB.FAMILIES)
ULP = 2.0 ** -23

# the look-up each family's test file performed on its own before it moved onto the helper
OLD_LOOKUP = {
    "kg_ig": lambda s: min(1e-5, s),
    "cpi_ig": lambda s: min(1e-5, max(ULP, s)),
    "vecmodal_ig": lambda s: min(1e-5, max(ULP, s)),
    "smooth_ig": lambda s: min(1e-4, s),
    "cv": lambda s: s,
    "vecmodal": lambda s: s,
    "seqcnn": lambda s: s,
}


def _file(name):
    return json.load(open(FB.FAMILIES[name].path))


def fresh(name):
    """A family like the table's with nothing measured, so that no test writes into what another reads."""
    f = FB.FAMILIES[name]
    return FB.Family(f.name, f.cap, f.floor, f.figure, f.strict)


def digits4(v):
    return "%.3e" % v


def test_the_table():
    assert NAMES == ["cpi_ig", "cv", "kg_ig", "seqcnn", "smooth_ig", "vecmodal", "vecmodal_ig"]
    assert {n: FB.FAMILIES[n].cap for n in NAMES} == {"kg_ig": 1e-5, "cpi_ig": 1e-5, "vecmodal_ig": 1e-5, "cv": 1e-5, "seqcnn": 1e-5,
                                                      "smooth_ig": 1e-4, "vecmodal": 1e-4}
    assert {n: FB.FAMILIES[n].floor for n in NAMES} == dict({n: ULP for n in NAMES}, vecmodal=2.0 ** -22)
    assert [n for n in NAMES if FB.FAMILIES[n].strict] == ["cpi_ig", "vecmodal_ig"]
    assert sum(len(_file(n)["bounds"]) for n in NAMES) == 150          # 149 and cpi_ig's completeness key
    for n in NAMES:
        assert os.path.basename(FB.FAMILIES[n].path) == n + "_bounds.json" and FB.FAMILIES[n].record_variable == "KGCN_%s_RECORD" % n.upper()


@pytest.mark.parametrize("name", NAMES)
def test_stored_bounds_follow_the_rule(name):
    """min(cap, stored) = min(cap, max(floor, 10 x measured)) for every stored key -- both sides under the cap because kg_ig's
    file stores values above it; equal to four significant digits because the hand-written files (cv, seqcnn, vecmodal) keep
    four, and exactly where the file keeps all of them."""
    f, table = FB.FAMILIES[name], _file(name)
    assert table["bounds"] and set(table["bounds"]) <= set(table["measured"])
    exact = name not in ("cv", "seqcnn", "vecmodal")
    for key, stored in table["bounds"].items():
        rule = min(f.cap, max(f.floor, 10.0 * table["measured"][key]))
        assert digits4(min(f.cap, stored)) == digits4(rule), (key, stored, rule)
        assert not exact or min(f.cap, stored) == rule, (key, stored, rule)
        assert stored >= ULP, key


@pytest.mark.parametrize("name", NAMES)
def test_the_helper_agrees_with_the_old_lookups(name):
    f = fresh(name)
    for key, stored in _file(name)["bounds"].items():
        if (name, key) == ("cpi_ig", "completeness excess / scale"):       # held to a literal 1e-5 before it had an entry
            assert f.bound(key) == 1e-5 == stored
            continue
        assert f.bound(key) == OLD_LOOKUP[name](stored), key
        assert f.stored(key) == stored


@pytest.mark.parametrize("name", NAMES)
def test_a_key_without_an_entry_is_refused_unless_the_run_records(name, monkeypatch, tmp_path):
    f = fresh(name)
    monkeypatch.delenv(f.record_variable, raising=False)
    for call in (f.bound, f.stored, lambda k: f.check(k, [1.0], [1.0]), lambda k: f.hold(k, 0.0)):
        with pytest.raises(KeyError) as e:
            call("no such key")
        assert "no such key" in str(e.value) and os.path.basename(f.path) in str(e.value)
    assert not f.measured
    monkeypatch.setenv(f.record_variable, str(tmp_path / "record.json"))
    assert f.bound("no such key") == f.cap and f.stored("no such key") is None
    f.check("no such key", [1.0], [1.0])
    with pytest.raises(AssertionError):
        f.check("no such key", [1.0 + 2.0 * f.cap], [1.0])              # the cap still holds
    known = next(iter(_file(name)["bounds"]))
    assert f.bound(known) == OLD_LOOKUP[name](_file(name)["bounds"][known])      # a recording run holds the known keys as any run


def test_error_figures():
    got, ref = np.array([[1.0, 2.5], [-4.0, 0.0]]), np.array([[1.0, 2.0], [-4.0, 0.0]])            # max |diff| 0.5, max|ref| 4
    small = ref / 8.0                                                                              # max |diff| 1.5 (got - small: 3.5), max|ref| 0.5
    assert FB.error_figure(got, ref, FB.OVER_REF) == 0.125
    assert FB.error_figure(got, ref, FB.OVER_REF_OR_TINY) == 0.125 == FB.rel_err(got, ref)
    assert FB.error_figure(got, ref, FB.OVER_ONE_OR_REF) == 0.125
    assert FB.error_figure(got, ref, FB.OVER_REF_OR_ABSOLUTE) == 0.125
    assert FB.error_figure(small + 0.25, small, FB.OVER_REF) == 0.5
    assert FB.error_figure(small + 0.25, small, FB.OVER_ONE_OR_REF) == 0.25                        # max(1, 0.5)
    assert FB.error_figure(got, ref, FB.OVER_REF, big=2.0) == 0.25                                 # big= in place of max|ref|
    assert FB.error_figure(got, ref, FB.OVER_REF_OR_TINY, absolute=True) == 0.5                    # absolute= : no division
    assert FB.error_figure(np.float32(3.0), 2.0, FB.OVER_REF_OR_TINY, absolute=True) == 1.0        # a scalar
    zero = np.zeros(3)
    assert FB.error_figure(zero + 0.25, zero, FB.OVER_REF_OR_ABSOLUTE) == 0.25                     # all-zero reference: absolute
    assert FB.error_figure(zero + 0.25, zero, FB.OVER_ONE_OR_REF) == 0.25
    assert FB.error_figure(zero + 0.25, zero, FB.OVER_REF_OR_TINY) == 0.25 / 1e-30
    assert FB.error_figure(zero + 0.25, zero, FB.OVER_REF) == np.inf                               # no bound admits it
    assert np.isnan(FB.error_figure(zero, zero, FB.OVER_REF))
    empty = np.zeros((2, 0, 3))
    assert FB.error_figure(empty, empty, FB.OVER_REF_OR_ABSOLUTE) == 0.0 == FB.error_figure(empty, empty, FB.OVER_REF_OR_TINY)
    for figure in (FB.OVER_REF, FB.OVER_ONE_OR_REF):
        with pytest.raises(ValueError):
            FB.error_figure(empty, empty, figure)


@pytest.mark.parametrize("name", NAMES)
def test_check_uses_the_family_figure_and_its_pre_assertions(name, capsys):
    f = fresh(name)
    key = next(iter(_file(name)["bounds"]))
    ref = np.array([0.5, -0.25, 0.0])
    off = 0.5 * f.bound(key) * (1.0 if f.figure == FB.OVER_ONE_OR_REF else 0.5)      # half the bound in the family's figure
    err = f.check(key, ref + off, ref, tag="a tag")
    assert err == FB.error_figure(ref + off, ref, f.figure) and err <= f.bound(key)
    line = capsys.readouterr().out.strip()
    assert line == "BOUND %s | %s | a tag | err / %s = %.3e | bound %.3e" % (name, key, f.figure, err, f.bound(key))
    with pytest.raises(AssertionError):
        f.check(key, ref + 4.0 * off, ref)                                           # twice the bound
    assert f.measured == {key: FB.error_figure(ref + 4.0 * off, ref, f.figure)}      # recorded before it is refused
    f.check(key, ref + off, ref)
    assert f.measured[key] > err                                                     # the largest stays
    zero = np.zeros(3)
    if f.strict:
        with pytest.raises(AssertionError):
            f.check(key, np.zeros((3, 1)), ref)                                      # a shape that only broadcasts
        with pytest.raises(AssertionError):
            f.check(key, [0.5, np.nan, 0.0], ref)
        with pytest.raises(AssertionError):
            f.check(key, zero, zero)                                                 # a reference that is all zero
    elif f.figure == FB.OVER_REF:
        with pytest.raises(AssertionError):
            f.check(key, zero, zero)                                                 # nan is not <= the bound
    else:
        f.check(key, zero, zero)
    if f.figure in (FB.OVER_REF_OR_ABSOLUTE, FB.OVER_REF_OR_TINY):
        f.check(key, np.zeros((0, 4)), np.zeros((0, 4)))                             # nothing to compare
    with pytest.raises(AssertionError):
        f.check(key, [0.5, np.nan, 0.0], ref)                                        # a NaN passes no family


def test_absolute_big_and_given_errors(capsys):
    f = fresh("smooth_ig")
    key = next(iter(_file("smooth_ig")["bounds"]))
    b = f.bound(key)
    f.check(key, 1000.0 + 500.0 * b, 1000.0)                                         # half the bound of |ref| ...
    with pytest.raises(AssertionError):
        f.check(key, 1000.0 + 500.0 * b, 1000.0, absolute=True)                      # ... 500 bounds as it stands
    g = fresh("vecmodal_ig")
    key = "fused vec check_score"
    b = g.bound(key)
    with pytest.raises(AssertionError):
        g.check(key, [0.01 + 0.02 * b], [0.01])                                      # two bounds of max|ref| ...
    g.check(key, [0.01 + 0.02 * b], [0.01], big=0.04)                                # ... half a bound of the given magnitude
    capsys.readouterr()
    h = fresh("kg_ig")
    key = "edge_loss completeness excess / scale"
    assert h.stored(key) == _file("kg_ig")["bounds"][key] < 1e-5
    h.hold(key, 0.9e-5, bound=max(1e-5, h.stored(key)))                              # a margin of the caller's own making
    assert "bound 1.000e-05" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        h.hold(key, 0.9e-5)
    assert h.measured == {key: 0.9e-5}


def test_a_recording_run_writes_the_largest_error_per_key_at_exit(tmp_path):
    record = tmp_path / "deep" / "record.json"
    script = ("import sys\nsys.path.insert(0, %r)\n" % os.path.dirname(os.path.abspath(__file__)) +
              "import family_bounds as FB\nf = FB.FAMILIES['seqcnn']\n"
              "f.check('dw', [1.0 + 1e-6], [1.0])\nf.check('dw', [1.0 + 2e-6], [1.0])\nf.check('dw', [1.0], [1.0])\n"
              "f.hold('a new key', 3e-6)\nFB.FAMILIES['cv'].check('loss_cost', 2.0, 2.0)\n")
    env = dict(os.environ, KGCN_SEQCNN_RECORD=str(record))
    env.pop("KGCN_CV_RECORD", None)
    subprocess.check_call([sys.executable, "-c", script], env=env, stdout=subprocess.DEVNULL)
    got = json.load(open(record))
    assert got == {"measured": {"dw": FB.error_figure([1.0 + 2e-6], [1.0], FB.OVER_REF_OR_ABSOLUTE), "a new key": 3e-6}}
    assert os.listdir(record.parent) == ["record.json"]                            # cv did not record: nothing of its own


@pytest.mark.parametrize("name", NAMES)
def test_regenerating_from_its_own_measurements_gives_the_file_back(name, tmp_path):
    f = FB.FAMILIES[name]
    before = _file(name)
    copy, record = str(tmp_path / "bounds.json"), str(tmp_path / "record.json")
    shutil.copy(f.path, copy)
    json.dump({"measured": before["measured"]}, open(record, "w"))
    subprocess.check_call([sys.executable, os.path.abspath(FB.__file__), name, record, copy], stdout=subprocess.DEVNULL)
    after = json.load(open(copy))
    assert list(after) == list(before) and after["measured"] == before["measured"]
    assert {k: v for k, v in after.items() if k not in ("bounds", "measured")} == \
        {k: v for k, v in before.items() if k not in ("bounds", "measured")}
    assert sorted(after["bounds"]) == sorted(before["bounds"])
    for key, stored in before["bounds"].items():                                     # see test_stored_bounds_follow_the_rule
        assert digits4(after["bounds"][key]) == digits4(min(f.cap, stored)), key
    assert _file(name) == before                                                     # the committed file was not touched


def test_the_command_refuses_an_unknown_family(tmp_path):
    r = subprocess.run([sys.executable, os.path.abspath(FB.__file__), "nobody", str(tmp_path / "r.json")], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr
