"""CPU tests: the run-time switches are declared once per layer — the library's table (emgraph_amd/csrc/emg_abi.hip), the Python
package's (emgraph_amd/_switches.py) — read only through those tables' readers, listed in DESIGN.md's table under the same names,
and, unless they are configuration, named by a test.  The sources are scanned as text."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emgraph_amd", "csrc")
SWITCHES_PY = os.path.join(ROOT, "emgraph_amd", "_switches.py")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _library_table():
    return re.findall(r'^\s*\{"(\w+)", SwitchDecl::(?:Int|Word), "', _read(os.path.join(CSRC, "emg_abi.hip")), re.M)


def _python_table():
    spec = importlib.util.spec_from_file_location("_emg_switches", SWITCHES_PY)   # (the file alone: no torch, no library)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _design_table():
    """name -> (layer, whole row) of DESIGN.md's switch table"""
    rows = re.findall(r"^\| `(\w+)` \| (library|Python|both) \|(.*)$", _read(os.path.join(ROOT, "DESIGN.md")), re.M)
    assert len(rows) == len({r[0] for r in rows}), "a switch is listed twice"
    return {name: (layer, rest) for name, layer, rest in rows}


def test_the_library_reads_its_environment_in_one_place():
    hits = [(os.path.basename(p), line.strip()) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p)
            for line in _read(p).splitlines() if "getenv" in line]
    assert hits == [("emg_abi.hip", "const char* e = getenv(kSwitches[s].name);")], hits
    assert re.search(r"const char\* sw_word\(Switch s\) \{\n    const char\* e = getenv\(", _read(os.path.join(CSRC, "emg_abi.hip")))


def test_the_library_table_follows_the_enum_and_every_switch_is_read():
    enum = re.search(r"enum Switch \{(.*?)\};", _read(os.path.join(CSRC, "emg_common.hpp")), re.S).group(1)
    ids = [x.strip() for x in enum.split(",") if x.strip()]
    assert ids[-1] == "SW_COUNT"
    assert ["EMG_" + x[3:] for x in ids[:-1]] == _library_table()
    used = "".join(_read(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    for x in ids[:-1]:
        assert re.search(r"sw_(int|word)\(%s\)" % x, used), "%s is declared and never read" % x


def test_the_library_has_no_compile_time_knobs_but_the_declared_ones():
    """EMG_TRACE (DESIGN.md "Compile-time:"), the build's EMG_SRC_HASH and the host / device split: a new conditional — an ablation
    macro, a tuning value behind #ifndef — has to be argued for here."""
    allowed = {"EMG_TRACE", "EMG_SRC_HASH", "__HIP_DEVICE_COMPILE__"}
    for p in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(p):
            for no, line in enumerate(_read(p).splitlines(), 1):
                m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
                if m:
                    names = set(re.findall(r"[A-Za-z_]\w*", m.group(2).split("//")[0])) - {"defined"}
                    assert names and names <= allowed, "%s:%d: %s" % (os.path.basename(p), no, line.strip())


def test_the_package_reads_its_environment_in_one_place():
    for p in glob.glob(os.path.join(ROOT, "emgraph_amd", "**", "*.py"), recursive=True):
        if os.path.abspath(p) != SWITCHES_PY:
            assert not re.search(r"\b(environ|getenv)\b", _read(p)), "%s reads the environment itself" % os.path.relpath(p, ROOT)


def test_the_python_table_declares_what_the_package_reads():
    mod = _python_table()
    read = set()
    for p in glob.glob(os.path.join(ROOT, "emgraph_amd", "**", "*.py"), recursive=True):
        read.update(re.findall(r'_switches\.get\("(\w+)"\)', _read(p)))
    assert read == set(mod.SWITCHES)
    with pytest.raises(KeyError):
        mod.get("EMG_NOT_DECLARED")


def test_design_md_lists_each_layers_switches():
    doc = _design_table()
    lib, py = set(_library_table()), set(_python_table().SWITCHES)
    assert lib and py
    assert {n for n, (layer, _) in doc.items() if layer in ("library", "both")} == lib
    assert {n for n, (layer, _) in doc.items() if layer in ("Python", "both")} == py
    assert {n for n, (layer, _) in doc.items() if layer == "both"} == lib & py


def test_every_switch_that_is_not_configuration_is_named_by_a_test():
    doc = _design_table()
    tests = "".join(_read(p) for p in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)
                    if os.path.abspath(p) != os.path.abspath(__file__))
    for name, (_, rest) in sorted(doc.items()):
        if "*configuration*" not in rest:
            assert re.search(r"\b%s\b" % name, tests), "%s ships without a test that names it" % name
