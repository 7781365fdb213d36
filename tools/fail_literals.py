#!/usr/bin/env python3
"""The messages the backend can report: every string literal in the argument
list of fail( and of the helpers that hand their message to it (alloc_upload;
compose.hpp's live, create_with_table, destroy_with_table, coeff_grid), plus the messages that a plan check
(plan_is, formerly plan_matches) composes as its `what` argument followed by a
suffix, over csrc/*.hip and csrc/*.hpp; sorted and de-duplicated, one per line.
A host refactor that must not move a message compares the output for the parent
commit's csrc directory with the output for its own:

    python tools/fail_literals.py PARENT_CSRC > before.txt
    python tools/fail_literals.py > after.txt
    diff before.txt after.txt
"""
import glob
import os
import re
import sys

CALLS = re.compile(r"\b(fail|alloc_upload|live|create_with_table|destroy_with_table|coeff_grid)\(")
LITERAL = re.compile(r'"((?:[^"\\]|\\.)*)"')
COMPOSERS = re.compile(r"\b(plan_is|plan_matches)\(")
SUFFIX = re.compile(r'std::string\(what\) \+ "([^"]*)"\)')


def arguments(text, start):
    """The text of the call whose opening parenthesis ends at `start`."""
    depth, i, in_str = 1, start, False
    while depth and i < len(text):
        c = text[i]
        if in_str:
            if c == "\\":
                i += 1
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
        elif c == "(":
            depth += 1
        elif c == ")":
            depth -= 1
        i += 1
    return text[start:i]


def literals(csrc):
    found, whats, suffixes = set(), set(), set()
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        text = open(path).read()
        for m in CALLS.finditer(text):
            found.update(LITERAL.findall(arguments(text, m.end())))
        for m in COMPOSERS.finditer(text):
            whats.update(LITERAL.findall(arguments(text, m.end())))
        suffixes.update(SUFFIX.findall(text))
    return sorted(found | {w + s for w in whats for s in suffixes})


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "upmem--openfhe_amd", "csrc")
    print("\n".join(literals(csrc)))
