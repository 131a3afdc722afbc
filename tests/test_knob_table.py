"""tests/_knobs.py against the library (no GPU: teo_tune_* is host state): one row per key of teo_tune_keys(), every value a GPU test
runs is accepted and reads back, one value outside each bounded set is refused, and every test a row names exists."""
import ast
import os

from teochat_amd import _lib as L
from tests._knobs import KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_has_one_row_per_library_key():
    keys = L.tune_keys()
    assert len(keys) == len(set(keys))
    assert set(KNOBS) == set(keys), (sorted(set(keys) - set(KNOBS)), sorted(set(KNOBS) - set(keys)))


def test_every_listed_value_is_accepted_and_reads_back_and_one_outside_is_refused():
    t = L.Tune()
    try:
        for key, row in KNOBS.items():
            assert row.contract in ("bitwise", "fp32_order"), key
            assert len(set(row.values)) == len(row.values) >= 2, key
            assert t.get(key) in row.values, (key, "the shipped default is among the values run")
            for v in row.values:
                assert t.try_set(key, v) == 0, (key, v)
                assert t.get(key) == v, (key, v)
            if row.reject is not None:
                before = t.get(key)
                assert t.try_set(key, row.reject) != 0, (key, row.reject)
                assert t.get(key) == before, key
            assert t.reset() == 0
    finally:
        t.close()


def _test_names(module):
    tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_named_test_exists_and_every_entry_point_is_exported():
    names = {}
    exports = set(L.EXPORTS)
    for key, row in KNOBS.items():
        assert row.tests, key
        for tid in row.tests:
            module, name = tid.split("::")
            if module not in names:
                names[module] = _test_names(module)
            assert name in names[module], (key, tid)
        for e in row.entry:
            assert e in exports, (key, e)
