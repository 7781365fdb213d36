#!/usr/bin/env python3
"""Is the gfx950 device code of two csrc directories the same, kernel by kernel?

    python tools/isa_diff.py PARENT_CSRC upmem--openfhe_amd/csrc

Each translation unit of the Makefile's SRCS is compiled device-only to
assembly (the Makefile's `asm` flags) in both trees; each directory must sit in
its tree (the sources include ../../include/ofhe_hip.h).  The assembly is cut
at function symbols, and every kernel's text -- instructions, its .amdhsa_kernel
descriptor, and its entry of the amdhsa.kernels metadata (registers, LDS,
scratch, argument layout) -- is compared by mangled name.  Local labels carry
the function's ordinal in the file, which a deleted kernel shifts, so the
ordinal is dropped (in labels and in the loop comments that cite them, with
the padding that aligns a label's comment); so are the __hip_cuid_ lines, a
hash of the source text, and the .section line that closes a function's text
by naming the next function.
What lies outside any function is compared as "(file scope)"; the file's
trailer (the code-end padding after the last function and what follows it, the
target and version lines after the last metadata entry) belongs to no kernel
and is left out, so a kernel does not change by ceasing to be the file's last.
Exit status 1 when a kernel differs or exists only in the second tree.

A change that adds kernels names them: `--new REGEX` (repeatable) lists the
kernels that exist only in the second tree and whose mangled name matches as
"new", without counting them:

    python tools/isa_diff.py PARENT_CSRC upmem--openfhe_amd/csrc \\
        --new 'k_block_add|k_sub_scale_add|k_square2'

A template that gained a defaulted parameter keeps its code and changes its
mangled name; `--rename REGEX REPL` (repeatable) rewrites the first tree's
assembly with re.sub before it is cut, so that such kernels are compared
under their new names:

    python tools/isa_diff.py PARENT_CSRC upmem--openfhe_amd/csrc \\
        --rename '(k_blockILi\\d+ELb[01]ELi\\d+ELi\\d+E)EE' '\\1Li1EEE'
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
MAKEFILE = os.path.join(HERE, "..", "upmem--openfhe_amd", "csrc", "Makefile")
BEGIN = re.compile(r"; -- Begin function (\S+)")  # on the symbol's .globl or .weak line
OBJECT = re.compile(r"^\s*\.type\s+\S+,@object")
NEXT_SECTION = re.compile(r"^\s*\.section\s+\.text\.")  # ends a function's text and names the next function
PAD = re.compile(r"\s+;")  # a label's comment is aligned by the label's length, ordinal included
CODE_END = re.compile(r"^\s*\.p2alignl\b")  # the padding after the file's last function; a .text line precedes it
ORDINAL = re.compile(r"(\.L(?:BB|func_(?:begin|end)|JTI|tmp|CPI)|\bBB(?=\d+_\d))\d+")  # BBn_m: loop comments


def make_var(name, default=None):
    m = re.search(rf"^{name}\s*[:?]?=\s*(.*)$", open(MAKEFILE).read(), re.M)
    return m.group(1).strip() if m else default


def assembly(csrc, src):
    arch = make_var("ARCH")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tu.s")
        subprocess.run([make_var("HIPCC"), "-O3", "-std=c++17", f"--offload-arch={arch}", "--cuda-device-only", "-S",
                        "-o", out, src], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    """{mangled name: text} of one assembly file, plus "(file scope)"."""
    text, _, meta = text.partition("amdhsa.kernels:\n")
    meta = meta.partition("\namdhsa.target:")[0]
    parts, name = {"(file scope)": []}, "(file scope)"
    for line in text.splitlines():
        if "__hip_cuid_" in line or NEXT_SECTION.match(line):
            continue
        if CODE_END.match(line):
            if parts[name] and parts[name][-1].strip() == ".text":
                parts[name].pop()
            break
        m = BEGIN.search(line)
        if m:
            name = m.group(1)
            parts[name] = []
        elif OBJECT.match(line):  # data objects follow the functions
            name = "(file scope)"
        parts[name].append(PAD.sub(" ;", ORDINAL.sub(r"\1", line)))
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        m = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if m:
            parts.setdefault(m.group(1), []).append(entry)
    return {k: "\n".join(v) for k, v in parts.items()}


def main(a, b, renames=(), new=()):
    srcs = make_var("SRCS").split()
    with ThreadPoolExecutor(os.cpu_count() or 1) as pool:
        texts = list(pool.map(lambda job: assembly(*job), [(d, s) for s in srcs for d in (a, b)]))
    for pattern, repl in renames:
        print(f"first tree renamed: {pattern} -> {repl}")
        texts[0::2] = [re.sub(pattern, repl, t) for t in texts[0::2]]
    bad = 0
    for i, src in enumerate(srcs):
        ka, kb = kernels(texts[2 * i]), kernels(texts[2 * i + 1])
        only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        named = [k for k in only_b if any(re.search(n, k) for n in new)]
        only_b = [k for k in only_b if k not in named]
        differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        print(f"{src}: {len(ka) - 1} and {len(kb) - 1} functions; with the file scope "
              f"{len(set(ka) & set(kb)) - len(differ)} identical, "
              f"{len(differ)} differ, {len(only_a)} only in the first tree, {len(only_b)} only in the second")
        for tag, names in (("differs", differ), ("only in first", only_a), ("only in second", only_b),
                           ("new", named)):
            for k in names:
                print(f"  {tag}: {k}")
        bad += len(differ) + len(only_b)
    return 1 if bad else 0


if __name__ == "__main__":
    args, renames, new = sys.argv[1:], [], []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append((args[i + 1], args[i + 2]))
        del args[i:i + 3]
    while "--new" in args:
        i = args.index("--new")
        new.append(args[i + 1])
        del args[i:i + 2]
    sys.exit(main(os.path.abspath(args[0]), os.path.abspath(args[1]), renames, new))
