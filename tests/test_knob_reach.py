"""A knob must reach the engine a test calls.  A context (gsa_ctx) reads its GSA_* knobs from the
environment once, when it is created, and the `engine` fixture is session-scoped: a test that takes
`engine` and sets a knob with monkeypatch.setenv changes nothing in that engine, runs the default
instance and passes.  Such a test must use the `knobs` fixture (tests/conftest.py), which also sets
the knob on the session engine.  monkeypatch.setenv stays right where the engine is created after it
(shard.gpu_batch_align, bench helpers).  Also: every knob a test names is one the library knows, and
the Python tuple of knob names is the library's list."""
import ast
import glob
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_CALLS = ("setenv", "delenv")
# GSA_* names that tests use and that are not library knobs: read by bench.py / the package loader
NOT_KNOBS = {"GSA_BENCH_REHEARSE", "GSA_LIB"}


def _gsa_literal(call):
    a = call.args[0] if call.args else None
    return isinstance(a, ast.Constant) and isinstance(a.value, str) and a.value.startswith("GSA_")


def _is_env_attr(node):
    """monkeypatch.setenv / monkeypatch.delenv"""
    return (isinstance(node, ast.Attribute) and node.attr in ENV_CALLS and isinstance(node.value, ast.Name)
            and node.value.id == "monkeypatch")


def _params(fn):
    a = fn.args
    return [x.arg for x in a.posonlyargs + a.args + a.kwonlyargs]


def _calls(fn):
    return [n for n in ast.walk(fn) if isinstance(n, ast.Call)]


def violations(source, filename="<test module>"):
    """Functions of a test module that take `engine` and set a literal GSA_* name in the environment
    only: directly, through a module-level helper that does (any depth), or by handing monkeypatch
    (or its setenv / delenv) to a module-level helper that sets literal GSA_* names through it."""
    tree = ast.parse(source, filename)
    funcs = {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}

    def direct(fn):
        return any(_is_env_attr(c.func) and _gsa_literal(c) for c in _calls(fn))

    def through_param(fn):
        """the helper sets literal GSA_* names through a callable (or a monkeypatch) it was handed"""
        ps = set(_params(fn))
        for c in _calls(fn):
            if not _gsa_literal(c):
                continue
            f = c.func
            if isinstance(f, ast.Name) and f.id in ps:
                return True
            if isinstance(f, ast.Attribute) and f.attr in ENV_CALLS and isinstance(f.value, ast.Name) and f.value.id in ps:
                return True
        return False

    def hands_monkeypatch(call):
        args = list(call.args) + [k.value for k in call.keywords]
        return any(_is_env_attr(a) or (isinstance(a, ast.Name) and a.id == "monkeypatch") for a in args)

    def bad(fn, seen):
        if direct(fn):
            return True
        for c in _calls(fn):
            if not (isinstance(c.func, ast.Name) and c.func.id in funcs) or c.func.id in seen:
                continue
            h = funcs[c.func.id]
            if hands_monkeypatch(c) and through_param(h):
                return True
            if bad(h, seen | {c.func.id}):
                return True
        return False

    return sorted(name for name, fn in funcs.items() if "engine" in _params(fn) and bad(fn, {name}))


def _test_modules():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py")))


def test_engine_tests_do_not_select_through_the_environment():
    found = {}
    for path in _test_modules():
        v = violations(open(path).read(), path)
        if v:
            found[os.path.relpath(path, ROOT)] = v
    assert not found, "these take the session `engine` and set GSA_* with monkeypatch: use `knobs`: %r" % found


def test_rule_catches_the_patterns_it_is_for():
    direct = '''
def test_a(engine, monkeypatch):
    monkeypatch.setenv("GSA_TRACE_BAND", "0")
    engine.run()
'''
    helper = '''
def _select(monkeypatch, ns):
    monkeypatch.setenv("GSA_KROW_NS", str(ns))

def _outer(monkeypatch, ns):
    _select(monkeypatch, ns)

def test_b(engine, monkeypatch):
    _outer(monkeypatch, 8)

def test_own_engine(monkeypatch):
    _select(monkeypatch, 8)
'''
    handed = '''
def _select(setter, ns):
    setter("GSA_KROW_NS", str(ns))

def test_c(engine, monkeypatch):
    _select(monkeypatch.setenv, 8)

def test_d(engine, knobs):
    _select(knobs, 8)

def test_e(engine, monkeypatch):
    monkeypatch.delenv("GSA_KROW_NS", raising=False)

def test_f(engine, monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "1")

def test_own_engine(monkeypatch):
    _select(monkeypatch.setenv, 8)
'''
    assert violations(direct) == ["test_a"]
    assert violations(helper) == ["test_b"]
    assert violations(handed) == ["test_c", "test_e"]


def _knob_literals(path):
    tree = ast.parse(open(path).read(), path)
    return {n.value for n in ast.walk(tree)
            if isinstance(n, ast.Constant) and isinstance(n.value, str) and re.fullmatch(r"GSA_[A-Z0-9_]+", n.value)}


def test_knob_names_in_tests_are_known():
    unknown = {}
    for path in _test_modules() + [os.path.join(ROOT, "tests", "conftest.py")]:
        u = _knob_literals(path) - set(gsa.KNOB_NAMES) - NOT_KNOBS
        if u:
            unknown[os.path.relpath(path, ROOT)] = sorted(u)
    assert not unknown, "not in the library's knob list (gsa_set_knob refuses them): %r" % unknown


def test_knob_tuple_is_the_librarys_list():
    text = open(os.path.join(ROOT, "gpuseqalign_amd", "csrc", "gsa_capi.hip")).read()
    m = re.search(r"kKnobNames\[\]\s*=\s*\{(.*?)\};", text, re.S)
    assert m, "kKnobNames not found in gsa_capi.hip"
    names = tuple(re.findall(r'"(GSA_[A-Z0-9_]+)"', m.group(1)))
    assert len(names) >= 20 and len(set(names)) == len(names)
    assert gsa.KNOB_NAMES == names
