"""The per-family accuracy bounds of the GPU tests, held in one place.

A family is one feature's set of GPU comparisons against its fp64 oracle.  Its bounds file, tests/golden/<family>_bounds.json,
stores per key the error measured on an MI355X (`measured`) and the bound made from it (`bounds`) by the project's rule,

    stored = min(cap, max(10 x measured, floor)),

and a comparison is held to  bound(key) = min(cap, max(ULP, stored[key])):  never looser than ten times the error it showed,
never looser than the family's written tolerance (cap), never tighter than one fp32 ulp.  A key the file does not know is an
error naming the key and the file -- except in a recording run of that family (KGCN_<FAMILY>_RECORD=<file> in the environment),
where the cap alone holds and  {"measured": {key: largest error}}  is written to <file> when the interpreter exits.

    import family_bounds
    FB = family_bounds.FAMILIES["cpi_ig"]
    FB.check(key, got, ref, tag="...")            # error figure of the family, recorded, printed, asserted
    FB.hold(key, err)                             # the same for an error the caller computed
    FB.bound(key), FB.stored(key)                 # the bound held / the file's own number

    python tests/family_bounds.py FAMILY RECORD.json [BOUNDS.json]

rewrites `bounds` and `measured` of the family's file (or of BOUNDS.json) from a record by the rule above; every other field
stays as it is.  tests/test_family_bounds.py checks this module and the seven committed files on the CPU."""
import atexit
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23                                   # one fp32 ulp: the outputs are fp32, no bound binds below it

# ---- the error figures: max |got - ref| over ... ------------------------------------------------------------------------------------
OVER_REF = "max|ref|"                              # a reference that is all zero gives inf or nan, which no bound admits
OVER_REF_OR_TINY = "max(1e-30, max|ref|)"          # an empty comparison is 0
OVER_ONE_OR_REF = "max(1, max|ref|)"
OVER_REF_OR_ABSOLUTE = "max|ref|, absolute where ref is all zero"      # an empty comparison is 0
_SCALE = {OVER_REF: lambda m: m, OVER_REF_OR_TINY: lambda m: max(1e-30, m), OVER_ONE_OR_REF: lambda m: max(1.0, m),
          OVER_REF_OR_ABSOLUTE: lambda m: m if m > 0 else 1.0}
_EMPTY_IS_ZERO = (OVER_REF_OR_TINY, OVER_REF_OR_ABSOLUTE)


def error_figure(got, ref, figure, absolute=False, big=None):
    """max |got - ref| over the figure's magnitude of ref; absolute: over nothing; big: over this magnitude in place of max|ref|
    (for a difference of two outputs: the outputs' own magnitude)."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    if ref.size == 0 and figure in _EMPTY_IS_ZERO:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref).max()
        if not absolute:
            err = err / _SCALE[figure](np.abs(ref).max() if big is None else big)
    return float(err)


def rel_err(got, ref):
    """max |got - ref| / max(1e-30, max|ref|), for comparisons that carry a written tolerance of their own."""
    return error_figure(got, ref, OVER_REF_OR_TINY)


# ---- a family: its file, its rule, what a run measured ------------------------------------------------------------------------------
class Family:
    def __init__(self, name, cap, floor, figure, strict=False):
        """cap: the family's written tolerance; floor: what the rule never stores below; figure: its error figure; strict: check()
        first asserts equal shapes, finite values and a reference that is not all zero."""
        self.name, self.cap, self.floor, self.figure, self.strict = name, cap, floor, figure, strict
        self.path = os.path.join(GOLDEN, name + "_bounds.json")
        self.record_variable = "KGCN_%s_RECORD" % name.upper()
        self.measured = {}
        self._stored = None

    @property
    def recording(self):
        return bool(os.environ.get(self.record_variable))

    def stored(self, key):
        """-> the number the bounds file stores for key; None in a recording run that meets a key without one."""
        if self._stored is None:
            self._stored = json.load(open(self.path))["bounds"] if os.path.exists(self.path) else {}
        if key not in self._stored:
            if self.recording:
                return None
            raise KeyError("no bound for %r in %s" % (key, self.path))
        return self._stored[key]

    def bound(self, key):
        stored = self.stored(key)
        return self.cap if stored is None else min(self.cap, max(ULP, stored))

    def hold(self, key, err, tag="", bound=None, figure="given"):
        """Record err under key (the largest stays), print key, error and bound on one line, assert err <= bound.  bound: what
        to hold it to in place of bound(key)."""
        bound = self.bound(key) if bound is None else bound
        self.measured[key] = max(self.measured.get(key, 0.0), err)
        print("BOUND %s | %s | %s | err / %s = %.3e | bound %.3e" % (self.name, key, tag, figure, err, bound))
        assert err <= bound, (self.name, key, tag, err, bound)
        return err

    def check(self, key, got, ref, tag="", absolute=False, big=None):
        ref = np.asarray(ref, np.float64)
        got = np.asarray(got, np.float64)
        if self.strict:
            assert got.shape == ref.shape, (key, got.shape, ref.shape)
            assert np.isfinite(got).all(), key
            assert np.abs(ref).max() > 0, key
        err = error_figure(got, ref, self.figure, absolute, big)
        return self.hold(key, err, tag, figure="1" if absolute else self.figure if big is None else "%.3e" % big)

    def write_record(self):
        path = os.environ.get(self.record_variable)
        if path and self.measured:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            json.dump({"measured": self.measured}, open(path, "w"), indent=1, sort_keys=True)


# caps: the written tolerances the files' own notes name.  floors: vecmodal's file was made with 2^-22 (two ulp of max(1, |ref|));
# its one floored entry, metric_sums, stores that number to four digits, 2.384e-07, a hair below 2^-22 itself -- which is why
# bound() floors every family at ULP and leaves the family's floor to the rule: no stored number moves when it is looked up.
FAMILIES = {f.name: f for f in (
    Family("kg_ig", 1e-5, ULP, OVER_REF),
    Family("cpi_ig", 1e-5, ULP, OVER_REF, strict=True),
    Family("vecmodal_ig", 1e-5, ULP, OVER_REF, strict=True),
    Family("smooth_ig", 1e-4, ULP, OVER_REF_OR_TINY),
    Family("cv", 1e-5, ULP, OVER_ONE_OR_REF),
    Family("vecmodal", 1e-4, 2.0 ** -22, OVER_ONE_OR_REF),
    Family("seqcnn", 1e-5, ULP, OVER_REF_OR_ABSOLUTE),
)}


@atexit.register
def _write_records():
    for family in FAMILIES.values():
        family.write_record()


def regenerate(family, record_path, bounds_path=None):
    """`bounds` and `measured` of the family's file from the record of a run: stored = min(cap, max(10 x measured, floor))."""
    f = FAMILIES[family]
    path = bounds_path or f.path
    measured = json.load(open(record_path))["measured"]
    table = json.load(open(path))
    table["measured"] = {k: measured[k] for k in sorted(measured)}
    table["bounds"] = {k: min(f.cap, max(10.0 * measured[k], f.floor)) for k in sorted(measured)}
    with open(path, "w") as out:
        json.dump(table, out, indent=1)
        out.write("\n")
    return table


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4) or sys.argv[1] not in FAMILIES:
        sys.exit("usage: python tests/family_bounds.py {%s} RECORD.json [BOUNDS.json]" % ",".join(FAMILIES))
    made = regenerate(*sys.argv[1:])
    print("%s: %d bounds written" % (sys.argv[1], len(made["bounds"])))
