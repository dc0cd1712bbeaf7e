"""The rule that keeps the helpers of the suite out of the test modules: what two test files share lives in a plain helper module
(cases.py, periodic2d_kinds.py, periodic2d_sweeps.py, a *_reference.py, ...), never in a test_*.py that another file imports."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_module_imports_a_test_module():
    """a test module imported as a library runs its module-level code twice under two names, and editing one of its constants
    silently redefines whatever the importer builds from it (the cases of a golden record, for instance)"""
    found = []
    paths = sorted(glob.glob(os.path.join(HERE, "*.py")) + glob.glob(os.path.join(HERE, "golden", "*.py")))
    assert len(paths) > 100
    for path in paths:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):      # (a relative import names the module among the aliases)
                names = [node.module or ""] + ([a.name for a in node.names] if node.level else [])
            found += [(os.path.relpath(path, HERE), node.lineno, name) for name in names if name.split(".")[-1].startswith("test_")]
    assert not found, found
