"""What barotp's host drivers (blom_amd/csrc/stage_barotp.hip, stage_barotp_pair.hip) say ONCE: which instantiations of the tiled
kernels there are (the shape dispatcher over kBtShapes), how a PairArgs starts out (bt_args), the phases' time weights (bt_schedule), and
the list of tile shapes the option barotp_tile accepts.  Checked on the sources, in the style of test_shared_definitions.py: a second
launcher with its own chain of shapes, a hand-filled PairArgs or a second copy of the weights goes unnoticed by every parity test until
the copies drift apart."""
import os
import re

from test_shared_definitions import CSRC, code

BAROTP = ("stage_barotp.hip", "stage_barotp_pair.hip", "blomgpu_internal.h")
DISPATCHER = "bt_shape_kernel"


def functions(src):
    """(name, start, end) of every brace block at file scope of a comment-stripped source, named by the last identifier in front of a
    `(` outside all parentheses of its head (a function's name), or by the head's last word (struct, enum)"""
    out, depth, start, head_from = [], 0, 0, 0
    for pos, ch in enumerate(src):
        if ch == "{":
            if depth == 0:
                start = pos
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth == 0:
                head, name, par = src[head_from:start], None, 0
                for m in re.finditer(r"(\w+)\s*\(|\(|\)", head):
                    if m.group(0) == ")":
                        par -= 1
                        continue
                    if par == 0 and m.group(1):
                        name = m.group(1)
                    par += 1
                out.append((name or (re.findall(r"\w+", head) or ["?"])[-1], start, pos))
                head_from = pos + 1
        elif ch == ";" and depth == 0:
            head_from = pos + 1
    return out


def enclosing(path, pattern):
    """names of the file-scope blocks of `path` in which `pattern` occurs, one entry per occurrence (None: at file scope)"""
    src = code(os.path.join(CSRC, path))
    fns = functions(src)
    return [next((n for n, a, b in fns if a <= m.start() <= b), None) for m in re.finditer(pattern, src)]


def test_the_block_finder_finds_the_functions():
    names = [n for n, _, _ in functions(code(os.path.join(CSRC, "stage_barotp_pair.hip")))]
    for n in ("k_bt_steps", "k_bt_steps4", "k_bt_halo3", DISPATCHER, "bt_form", "bt_run_pairs", "bt_run_blocked", "PairArgs"):
        assert names.count(n) == 1, (n, names)


def test_kernel_instantiations_are_named_in_the_shape_dispatcher_only():
    """k_bt_steps<...> / k_bt_steps4<...> with explicit arguments: inside the dispatcher, and in the explicit instantiations at file scope
    that pin the order of the device code"""
    for path in BAROTP:
        where = enclosing(path, r"\bk_bt_steps4?\s*<")
        assert set(where) <= {DISPATCHER, None}, (path, where)
        src = code(os.path.join(CSRC, path))
        for m in re.finditer(r"^.*\bk_bt_steps4?\s*<.*$", src, re.M):
            if not any(a <= m.start() <= b for _, a, b in functions(src)):
                assert re.match(r"\s*BT_INSTANTIATE\(", m.group(0)), (path, m.group(0))
    assert DISPATCHER in enclosing("stage_barotp_pair.hip", r"\bk_bt_steps\s*<") and DISPATCHER in enclosing("stage_barotp_pair.hip", r"\bk_bt_steps4\s*<")


def test_a_pairargs_object_is_declared_in_one_function_only():
    where = [w for path in BAROTP for w in enclosing(path, r"\bPairArgs\s+\w+\s*(?:;|=|\{)")]
    assert where == ["bt_args"], where


def test_the_time_weights_are_formed_in_one_function_only():
    """the four expressions of phy/mod_barotp.F90:352-360 that divide by lstep, once each"""
    where = [w for path in BAROTP for w in enclosing(path, r"/\s*lstep\b")]
    assert where == ["bt_schedule"] * 4, where


def test_the_refusal_strings_list_the_tables_shapes():
    hdr = code(os.path.join(CSRC, "blomgpu_internal.h"))
    table = re.search(r"kBtShapes\s*\[\s*BT_NSHAPES\s*\]\s*=\s*\{(.*?)\}\s*;", hdr, re.S)
    assert table, "blomgpu_internal.h: no kBtShapes"
    shapes = sorted(100 * int(ti) + int(tj) for ti, tj in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,", table.group(1)))
    assert len(shapes) == 7 and int(re.search(r"BT_NSHAPES\s*=\s*(\d+)", hdr).group(1)) == 7
    for path, head in (("api.hip", "blomgpu_set_int: barotp_tile must be 0, "), ("stage_barotp_pair.hip", "barotp: tile shape must be ")):
        msgs = re.findall(r'"%s([^"]*)"' % re.escape(head), open(os.path.join(CSRC, path)).read())
        assert len(msgs) == 1, (path, msgs)
        assert sorted(int(x) for x in re.findall(r"\d+", msgs[0])) == shapes, (path, msgs[0], shapes)
    # ... and the validator reads the table instead of a list of its own
    api = code(os.path.join(CSRC, "api.hip"))
    assert not re.search(r"\b(3216|3208|1608|4016|2616|2615|4015)\b", re.sub(r'"[^"\n]*"', '""', api))
