"""Where the package forks and joins streams, read from its source (no table of line numbers to keep in step)."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tam_gcn_amd')
FORK_ATTRS = ('on', 'refork', 'mark', 'wait', 'join', '__exit__')
OTHER_FILES = ('training.py', 'inference.py', 'streaming.py', os.path.join('feeder', 'feeder_nucla_gcn.py'))


def _tree(rel):
    with open(os.path.join(PKG, rel)) as f:
        return ast.parse(f.read())


def functional_sites():
    """[(function, method, line)] of every call of a functional.Fork method on a local named `fk`, in source order."""
    out = []
    for fn in ast.walk(_tree('functional.py')):
        if isinstance(fn, ast.FunctionDef):
            for node in ast.walk(fn):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in FORK_ATTRS \
                        and isinstance(node.func.value, ast.Name) and node.func.value.id == 'fk':
                    out.append((fn.name, node.func.attr, node.lineno))
    return sorted(set(out), key=lambda s: s[2])


def site(function, method, k=0):
    """'functional.py:<line>' of the k-th call of `method` inside `function`."""
    lines = [ln for fn, attr, ln in functional_sites() if fn == function and attr == method]
    return f'functional.py:{lines[k]}'


def other_sites():
    """[(file, line)] of the hand-written wait_stream calls outside functional.py."""
    out = []
    for rel in OTHER_FILES:
        for node in ast.walk(_tree(rel)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'wait_stream':
                out.append((rel, node.lineno))
    return sorted(out)
