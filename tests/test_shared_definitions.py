"""What the translation units of blom_amd/csrc have to agree on is defined ONCE: the reference's constants (constants.h), the thread
prologue (the two macros of blomgpu_internal.h), the work-space slots (workspace_slots.h) and the prototypes of functions another file
defines (blomgpu_internal.h, hor3map_internal.h).  Checked on the sources, in the style of test_side_by_side_sets.py: a second copy can
change bits in one stage only, or make two kernels that run side by side share a slot, without any other test noticing."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kernel_rw_sets import rw_sets  # noqa: E402

CSRC = os.path.join(ROOT, "blom_amd", "csrc")
FILES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
CONSTANTS = "GRAV SPCIFH T0DEG ALPHA0 RHO0 PI_BLOM EPSILP EPSILT SPVAL ONEM ONECM ONEMM ONEMU".split()
GUARDED = re.compile("GRAV|ONEM|ONECM|ONEMM|ONEMU|EPSILP|EPSILT|ALPHA0|RHO0|SPCIFH|T0DEG|SPVAL", re.I)
# a module's own parameter whose name merely contains one of the above: mod_difest's drho0 (a density difference, not the reference density)
OWN = {"DRHO0"}
NUMBER = r"\(?\s*[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?\s*\)?"


def code(path):
    """the file without its comments (same length: offsets stay)"""
    blank = lambda m: re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r"//[^\n]*", blank, re.sub(r"/\*.*?\*/", blank, open(path).read(), flags=re.S))


def bindings(src):
    """(name, value text) of every #define NAME value and of every NAME = value of a `constexpr double` / `const double` declaration"""
    out = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+([^\n]*)$", src, re.M)]
    for m in re.finditer(r"\b(?:constexpr|const)\s+double\s+([^;]*);", src):
        out += [(b.group(1), b.group(2).strip()) for b in re.finditer(r"(\w+)\s*=\s*([^,]*)", m.group(1))]
    return out


def test_the_reference_constants_are_defined_once():
    own = bindings(code(os.path.join(CSRC, "constants.h")))
    for name in CONSTANTS:
        assert [n for n, _ in own].count(name) == 1, name
    for path in FILES:
        if os.path.basename(path) == "constants.h":
            continue
        for name, value in bindings(code(path)):
            assert name not in CONSTANTS, f"{os.path.basename(path)}: a second definition of {name}"
            assert not (GUARDED.search(name) and name not in OWN and re.fullmatch(NUMBER, value)), \
                f"{os.path.basename(path)}: {name} = {value} spells a shared constant out again: take it from constants.h"


def macros(src):
    return [(m.group(1), m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)((?:[^\n]*\\\n)*[^\n]*)", src, re.M)]


def test_the_thread_prologue_is_defined_once():
    found = []
    for path in FILES:
        for name, body in macros(code(path)):
            if "% (V).ni - (NBDY - 1)" in body:
                found.append((os.path.basename(path), name))
    assert sorted(found) == [("blomgpu_internal.h", "THREAD_IJ_NATURAL"), ("blomgpu_internal.h", "THREAD_IJ_XCD")], found


SLOT_NAME = r"(?:S2_\w+|N_DP|N_S|N_T|N_TR|R_BASE|R_DP|R_T|R_S|R_TR|F_BASE)"


def test_slot_names_are_defined_in_the_slot_header_only():
    for path in FILES:
        if os.path.basename(path) == "workspace_slots.h":
            continue
        src = code(path)
        bad = [n for n, _ in macros(src) if re.fullmatch(SLOT_NAME + r"|R_\w+", n)]
        # enum members at file scope (column 0): a kernel's own enums of register names (stage_momtum_fused.hip) are not slots
        for m in re.finditer(r"^enum\s*\w*\s*\{([^}]*)\}", src, re.M):
            bad += re.findall(r"\b(%s)\b" % SLOT_NAME, m.group(1))
        assert not bad, f"{os.path.basename(path)}: {bad} belong in workspace_slots.h"


def test_no_work_space_slot_is_a_bare_number():
    for path in FILES:
        src = code(path)
        bad = re.findall(r"\bWK2?\(\s*\w+\s*,\s*\d+\s*\)", src)
        assert not bad, f"{os.path.basename(path)}: {bad}"


PROTO = re.compile(r"^(?:static\s+|inline\s+|const\s+|unsigned\s+|struct\s+)*[A-Za-z_][\w:<>]*[\s\*&]+(\w+)\s*\((?:[^;{}()]|\([^()]*\))*\)\s*;", re.M)


def test_no_hip_file_declares_another_files_function():
    for path in FILES:
        if not path.endswith(".hip"):
            continue
        src = code(path)
        for m in PROTO.finditer(src):
            name = m.group(1)
            defined = re.search(r"\b%s\s*\((?:[^;{}()]|\([^()]*\))*\)\s*(?:const\s*)?\{" % name, src)
            assert defined, f"{os.path.basename(path)}: prototype of {name}, which another file defines: declare it in blomgpu_internal.h"


def side_by_side_kernels():
    from test_side_by_side_sets import WINDOWS
    ks = {fk for _, side, main, _ in WINDOWS for fk in side + main}
    text = open(os.path.join(ROOT, "tests", "test_thermf_cesm_host.py")).read()
    ks |= set(re.findall(r'"(stage_\w+\.hip)"\)?,\s*"(k_\w+)"', text))
    return sorted(ks)


@pytest.mark.parametrize("f,k", side_by_side_kernels())
def test_slots_of_the_side_by_side_kernels_resolve_to_numbers(f, k):
    """two names for one number cannot clash in test_side_by_side_sets.py: what it compares must be numbers"""
    r, w = rw_sets(os.path.join(CSRC, f), k)
    slots = [x for x in r | w if x.startswith(("wk:", "wk2:"))]
    assert all(x.split(":")[1].isdigit() for x in slots), (f, k, slots)


def test_the_kernel_list_is_not_empty():
    ks = side_by_side_kernels()
    assert len(ks) >= 25 and ("stage_thermf_cesm.hip", "k_thermf_cesm_flux") in ks and ("stage_momtum_fused.hip", "k_mom_visc_march") in ks
