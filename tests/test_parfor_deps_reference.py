"""Parfor dependency analysis against the reference's own expectations: every case of
ParForDependencyAnalysisTest.java (script, expected "dependency detected") is run through
compiler/parfor_deps.py.  The reference marks parfor32c's detected dependency as a false
positive of its own analysis ("32c: dep (no, dep is false positive)"); the linear analysis
here proves it independent.  parfor48b is a validation error (matrix loop bound), raised by
the translator rather than the dependency analysis."""
import json
import os
import re

import pytest

from systemml_amd.api.executor import compile_script
from systemml_amd.compiler.parfor_deps import check_program
from systemml_amd.parser.dml_parser import parse_dml
from systemml_amd.parser.errors import LanguageError

REF = "/root/reference/src/test"
JAVA = os.path.join(REF, "java/org/apache/sysml/test/integration/functions/parfor/ParForDependencyAnalysisTest.java")
SCRIPTS = os.path.join(REF, "scripts/functions/parfor")
KNOWN = {"parfor32c.dml": "reference false positive", "parfor48b.dml": "translator validation error"}


# the (script, expected) pairs of the Java test, stored so that the cases and their ids are the
# same whether or not the reference tree is present; the scripts themselves are read from it
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parfor_deps_cases.json")) as _f:
    CASES = [tuple(c) for c in json.load(_f)]


@pytest.mark.parametrize("script,expected", CASES)
def test_dependency_analysis_matches_reference(script, expected):
    path = os.path.join(SCRIPTS, script)
    if not os.path.exists(path):
        pytest.skip("reference test sources not mounted")
    src = open(path).read()
    try:
        check_program(parse_dml(src, path))
        got = "false"
    except LanguageError:
        got = "true"
    if script in KNOWN:
        assert got == "false"
        if script == "parfor48b.dml":
            with pytest.raises(LanguageError, match="must be a scalar"):
                compile_script(src)
        return
    assert got == expected, script


def test_parity_count():
    assert len(CASES) >= 70
    if os.path.exists(JAVA):     # the stored list is the Java test's own list
        assert CASES == re.findall(r'runTest\("(\w+\.dml)", (true|false)\)', open(JAVA).read())


def test_scalar_accumulation_is_an_output_dependency():
    # the reference accumulates matrices only; a scalar `s += ...` in a parfor body
    # is an output dependency (ParForStatementBlock.rCheckCandidates)
    with pytest.raises(LanguageError):
        compile_script("s = 0\nparfor (i in 1:4) { s += i }\nprint(s)")
    compile_script("A = matrix(0, 2, 2)\nparfor (i in 1:4) { A += i }\nprint(sum(A))")
