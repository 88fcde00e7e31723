"""Compare two AMDGPU assembly listings (hipcc -S --cuda-device-only) function by function: did a change to the sources change
the code of a kernel it was not meant to touch?

    python tools/isa_compare.py BEFORE.s AFTER.s [--hot NAME,NAME,... | --hot-all-but NAME,...] [--json OUT.json]

Per function: code bytes, vgpr_count, sgpr_count, vgpr_spill_count, private_segment_fixed_size and group_segment_fixed_size of
either side (kernels: the code object's metadata; a plain device function has no metadata: NumVgprs / ScratchSize of its
info block), and whether the instruction text is identical.  The text is compared after dropping `;` comments, assembler
directives and the function number of the .LBB labels (it follows the function's position in the file).  Functions are paired
by mangled name; one whose parameter types were renamed is paired by its name and literal template arguments.  Exit status 0;
the table is the result.  --hot names the functions (every instance of a template) that must not change, --hot-all-but the only
ones that may: each row then says whether it is in that hot set, and the last line counts the hot set's identical functions."""
import argparse
import json
import re
import sys

FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def normalised(body):
    out = []
    for line in body.split("\n"):
        line = line.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return "\n".join(out)


def parse(path):
    text = open(path).read()
    funcs = {}
    starts = list(re.finditer(r"^(\w+):\s*; @\1\n", text, re.M))
    for k, m in enumerate(starts):
        stop = starts[k + 1].start() if k + 1 < len(starts) else len(text)
        end = re.compile(r"^\.Lfunc_end\d+:\n", re.M).search(text, m.end(), stop)
        if not end:
            continue
        name, body, tail = m.group(1), text[m.end():end.start()], text[end.end():stop]
        info = {"text": normalised(body)}
        n = re.search(r"codeLenInByte = (\d+)", tail)
        info["code_bytes"] = int(n.group(1)) if n else None
        v, s = re.search(r"; NumVgprs: (\d+)", tail), re.search(r"; ScratchSize: (\d+)", tail)
        info["vgpr_count"] = int(v.group(1)) if v else None
        info["private_segment_fixed_size"] = int(s.group(1)) if s else None
        funcs[name] = info
    meta = text.split("amdhsa.kernels:", 1)
    if len(meta) == 2:
        for chunk in re.split(r"^  - ", meta[1], flags=re.M)[1:]:
            kv = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)$", chunk, re.M))
            f = funcs.get(kv.get("name"))
            if f is not None:
                for k in FIELDS:
                    if k in kv:
                        f[k] = int(kv[k])
    return funcs


def loose_name(mangled):
    """name and literal template arguments of a function in the anonymous namespace, without its parameter types"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return mangled
    start = m.end()
    end = start + int(m.group(1))
    t = re.match(r"I(?:L[a-z]\d+E)+E", mangled[end:])
    return mangled[start:end] + (t.group(0) if t else "")


def base_name(mangled):
    return re.sub(r"I(?:L[a-z]\d+E)+E$", "", loose_name(mangled))


def pair(a, b):
    pairs = [(n, n) for n in a if n in b]
    only_a = {loose_name(n): n for n in a if n not in b}
    only_b = {loose_name(n): n for n in b if n not in a}
    pairs += [(only_a[k], only_b[k]) for k in only_a if k in only_b]
    left = [only_a[k] for k in only_a if k not in only_b], [only_b[k] for k in only_b if k not in only_a]
    return pairs, left


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--json", default=None, help="also write the table as JSON")
    ap.add_argument("--hot", default=None, help="comma-separated function names: the hot set")
    ap.add_argument("--hot-all-but", default=None, help="comma-separated function names: the hot set is every other function")
    args = ap.parse_args()
    a, b = parse(args.before), parse(args.after)
    pairs, (gone, new) = pair(a, b)
    rows = []
    for na, nb in pairs:
        fa, fb = a[na], b[nb]
        row = {"function": nb, "identical": fa["text"] == fb["text"]}
        if args.hot is not None:
            row["hot_set"] = base_name(nb) in args.hot.split(",")
        elif args.hot_all_but is not None:
            row["hot_set"] = base_name(nb) not in args.hot_all_but.split(",")
        if na != nb:
            row["function_before"] = na
        for k in ("code_bytes",) + FIELDS:
            row[k] = [fa.get(k), fb.get(k)]
        rows.append(row)
    short = {"code_bytes": "bytes", "vgpr_count": "vgpr", "sgpr_count": "sgpr", "vgpr_spill_count": "spill",
             "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}
    print("%-9s %s  function" % ("identical", "  ".join("%15s" % short[k] for k in short)))
    for r in rows:
        cells = "  ".join("%15s" % ("%s -> %s" % tuple("-" if v is None else v for v in r[k])) for k in short)
        print("%-9s %s  %s%s" % ("yes" if r["identical"] else "NO", cells, r["function"], "  [hot]" if r.get("hot_set") else ""))
    for n in gone:
        print("only in %s: %s" % (args.before, n))
    for n in new:
        print("only in %s: %s" % (args.after, n))
    print("%d functions compared, %d identical, %d differ, %d only before, %d only after"
          % (len(rows), sum(r["identical"] for r in rows), sum(not r["identical"] for r in rows), len(gone), len(new)))
    hot = [r for r in rows if r.get("hot_set")]
    if args.hot is not None or args.hot_all_but is not None:
        print("hot set: %d functions, %d identical" % (len(hot), sum(r["identical"] for r in hot)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"before": args.before, "after": args.after, "functions": rows, "only_before": gone, "only_after": new,
                       "hot_set": len(hot), "hot_set_identical": sum(r["identical"] for r in hot)}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
