"""Launch names of the library (helper for the dispatch tests): every name a launch can carry in the per-launch record
(`_lib.launch_profile`), parsed from gcnn_capi.hip -- every literal in the initialiser of a kernel table (`static RowProgram<...>`,
`static EdgeKernel<...>`: the row programs and the edge passes) and the first argument of each `ProfScope` (the other launches),
with both sides of a `?:` (nested ones included).  The launch function's own `ProfScope` takes a parameter and carries no literal."""
from __future__ import annotations

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc", "gcnn_capi.hip")

_START = re.compile(r"\bProfScope\s+\w+\s*\(")
_TABLE = re.compile(r"\bstatic\s+(?:RowProgram|EdgeKernel)<[^;]*;")   # a table's declaration up to the end of its initialiser
_STRING = re.compile(r'"((?:[^"\\]|\\.)*)"')


def _first_argument(src: str, at: int) -> str:
    """Text of the call's first argument; `at` is just past its opening parenthesis.  Commas inside strings, parentheses and
    angle-bracket-free C expressions do not end it."""
    depth, i = 0, at
    while i < len(src):
        ch = src[i]
        if ch == '"':
            i = _STRING.match(src, i).end()
            continue
        if ch == "(":
            depth += 1
        elif ch == ")":
            if depth == 0:
                return src[at:i]
            depth -= 1
        elif ch == "," and depth == 0:
            return src[at:i]
        i += 1
    raise ValueError("unterminated call")


def launch_names(path: str = CAPI) -> set[str]:
    src = open(path).read()
    src = re.sub(r"//[^\n]*", "", src)   # comments quote names too
    names = {n for t in _TABLE.findall(src) for n in _STRING.findall(t)}
    for m in _START.finditer(src):
        names.update(_STRING.findall(_first_argument(src, m.end())))
    return names
