#!/usr/bin/env python3
"""Two device listings of `make -C nbodysim_amd/csrc asm`, compared function by function: did a change leave the kernels alone?

    python tools/listing_diff.py OLD.s NEW.s [--pad-false] [--drop-pack-types] [--allow REGEX ...] [--diff]

    (OLD.s, NEW.s: build/asm/nb_capi-hip-amdgcn-amd-amdhsa-gfx950.s of the two trees)

A function is what stands between the label of a symbol declared `.type NAME,@function` and the next `.Lfunc_end` (data labels
are not functions).  Of its lines the instructions and the block labels are kept: comments and directives go, the function
number in block labels (.LBB12_3 -> .LBB_3) goes, and a mangled symbol is replaced by its demangled name without the parameter
list.  Functions are paired by that name (c++filt); --pad-false lets a name that found no partner try again with `false`
appended to its template arguments, so that tree_walk_group<true> of a tree before a flag was added pairs with
tree_walk_group<true, false> of the tree after it; --drop-pack-types lets it first shed its trailing template arguments that are
types (a deduced parameter pack: tree_walk<1, true, true, false, float4 const*> -> tree_walk<1, true, true, false>).  One line per
function:

    identical      the kept lines are equal
    same opcodes   the first words of the instructions are equal, in order; operands, registers or offsets differ
    different      neither; followed by the difference of the two opcode multisets (-n old only, +n new only)

then the functions without a partner and a count.  --diff prints the unified diff of the kept lines under every pair that is
not identical.  Exit status 1 when a function is `different` or without a partner and no --allow REGEX matches its name.
The comparison is one of text: the tool knows no instruction.
"""
import argparse
import collections
import difflib
import re
import subprocess
import sys

MANGLED = re.compile(r"\b_Z[\w$.]+")


def plain_name(demangled: str) -> str:
    """`void ns::f<1, true>(float*, int) [clone x]` -> `ns::f<1, true>`: the parameter list and the return type go."""
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", demangled)
    if s.endswith(")") or s.endswith(") const"):                      # the parameter list: the last balanced (...) group
        depth, i = 0, s.rindex(")")
        while i >= 0:
            depth += (s[i] == ")") - (s[i] == "(")
            if depth == 0:
                break
            i -= 1
        s = s[:i]
    depth, cut = 0, 0                                                     # the return type: up to the last space outside <> and ()
    for i, c in enumerate(s):
        depth += (c in "<(") - (c in ">)")
        if c == " " and depth == 0:
            cut = i + 1
    return s[cut:]


def demangle(symbols):
    symbols = sorted(symbols)
    if not symbols:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout
    return {m: plain_name(d) for m, d in zip(symbols, out.splitlines())}


def functions(text: str) -> dict:
    """{plain name: kept lines} of one listing."""
    lines = text.splitlines()
    is_function = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    names = demangle(set(MANGLED.findall(text)))
    out, cur = {}, None
    for raw in lines:
        line = raw.split(";")[0].strip()
        if not line:
            continue
        if cur is None:
            if line.endswith(":") and line[:-1] in is_function:
                cur = out.setdefault(names.get(line[:-1], line[:-1]), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        elif line.startswith(".LBB") or not line.startswith("."):
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            cur.append(MANGLED.sub(lambda m: names[m.group(0)], " ".join(line.split())))
    return out


def opcodes(kept):
    return [l.split()[0] for l in kept if not l.endswith(":")]


VALUE = re.compile(r"true|false|-?\d\w*|\(.*\)-?\d+")


def without_pack_types(name: str) -> str:
    """`f<1, true, float const*, float>` -> `f<1, true>`: the trailing template arguments that are types and not values go."""
    if not name.endswith(">"):
        return name
    depth, cuts = 0, []
    for i in range(len(name) - 1, -1, -1):                              # the last <...> group and its top-level commas
        depth += (name[i] in ">)") - (name[i] in "<(")
        if depth == 1 and name[i] == ",":
            cuts.append(i)
        if depth == 0:
            break
    bounds = [i] + cuts[::-1] + [len(name) - 1]
    args = [name[x + 1:y].strip() for x, y in zip(bounds, bounds[1:])]
    while args and not VALUE.fullmatch(args[-1]):
        args.pop()
    return name[:i] + ("<" + ", ".join(args) + ">" if args else "")


def repair(a: dict, b: dict, drop_pack_types: bool, pad_false: bool) -> None:
    """Rename in place the names of one side that have no partner and gain one without their trailing type arguments
    (--drop-pack-types) or with `false` template arguments appended (--pad-false)."""
    for mine, other in ((a, b), (b, a)):
        for name in [n for n in mine if n not in other and n.endswith(">")]:
            tries = [without_pack_types(name)] if drop_pack_types else [name]
            for _ in range(4 if pad_false and tries[-1].endswith(">") else 0):
                tries.append(tries[-1][:-1] + ", false>")
            for t in tries:
                if t != name and t in other and t not in mine:
                    mine[t] = mine.pop(name)
                    break


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--pad-false", action="store_true")
    ap.add_argument("--drop-pack-types", action="store_true")
    ap.add_argument("--allow", action="append", default=[], metavar="REGEX")
    ap.add_argument("--diff", action="store_true")
    args = ap.parse_args(argv)
    a, b = (functions(open(p).read()) for p in (args.old, args.new))
    repair(a, b, args.drop_pack_types, args.pad_false)
    allowed = lambda name: any(re.search(r, name) for r in args.allow)
    count, bad = collections.Counter(), 0
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            verdict = "identical"
        elif opcodes(a[name]) == opcodes(b[name]):
            verdict = "same opcodes"
        else:
            verdict = "different"
        count[verdict] += 1
        line = f"{verdict:13s} {name}"
        if verdict == "different":
            ca, cb = collections.Counter(opcodes(a[name])), collections.Counter(opcodes(b[name]))
            line += " :" + "".join(f" -{n} {op}" for op, n in sorted((ca - cb).items())) + "".join(f" +{n} {op}" for op, n in sorted((cb - ca).items()))
            bad += not allowed(name)
        print(line)
        if args.diff and verdict != "identical":
            print("\n".join("    " + l for l in difflib.unified_diff(a[name], b[name], "old", "new", lineterm="", n=2)))
    for side, mine, other in (("old", a, b), ("new", b, a)):
        for name in sorted(set(mine) - set(other)):
            count["unpaired"] += 1
            bad += not allowed(name)
            print(f"{'only in ' + side:13s} {name}")
    print(f"{len(a)} functions in old, {len(b)} in new: " + ", ".join(f"{count[k]} {k}" for k in ("identical", "same opcodes", "different", "unpaired")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
