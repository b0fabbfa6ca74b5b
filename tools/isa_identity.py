"""Do two builds of a translation unit carry the same device code?  Compares, function by function, the gfx950 assembly that
`hipcc -save-temps=obj` leaves behind (the check behind a refactor that must not move an instruction, profiles/strip_shared_header.txt):
    python tools/isa_identity.py OLD.s NEW.s [OLD2.s NEW2.s ...] [--alias OLD_NAME_PART=NEW_NAME_PART ...]
A function = its label up to .Lfunc_end, plus the .amdhsa_* lines of its kernel descriptor.  Before the comparison comments, .file /
.ident / section directives and the __hip_cuid_ symbol go, mangled names become SYM and .LBB<n>_<m> loses the function index n.
Functions are matched by mangled name; --alias matches a renamed one (a part of the old name, mangled or demangled, against a part of the new one).
Prints a table (instructions, identical?, VGPR / AGPR / LDS / scratch of both builds); exit status 1 unless every function of OLD has
an identical partner and NEW has no function of its own."""
import re
import subprocess
import sys

RES = [("NumVgprs", "vgpr"), ("NumAgprs", "agpr"), ("LDSByteSize", "lds"), ("ScratchSize", "scratch")]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        dm = dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        dm = {n: n for n in names}
    return {n: short_name(n) if d == n else d for n, d in dm.items()}


def short_name(mangled):
    """ns::name<int, ...> of _ZN<len>ns<len>name[ILi<n>E...E]..., for names the demangler does not know (bf16 arguments: DF16b)"""
    m = re.match(r"_ZN(\d+)", mangled)
    parts, pos = [], 3
    while m:
        pos += len(m.group(1))
        parts.append(mangled[pos:pos + int(m.group(1))])
        pos += int(m.group(1))
        m = re.match(r"(\d+)", mangled[pos:])
    if not parts:
        return mangled
    t = re.match(r"I((?:Li\d+E)+)E", mangled[pos:])
    return "::".join(parts) + ("<%s>" % ", ".join(re.findall(r"Li(\d+)E", t.group(1))) if t else "")


def label(demangled):
    """the name without its argument list; "(anonymous namespace)::" goes first, or the cut at the first parenthesis leaves nothing"""
    return re.sub(r"\(.*", "", demangled.replace("(anonymous namespace)::", ""))


def norm(line):
    line = line.split(";")[0].rstrip()
    s = line.strip()
    if not s or s.startswith((".file", ".ident", ".section", ".text", ".type", ".size", ".globl", ".weak", ".protected", ".hidden")) or "__hip_cuid_" in s:
        return None
    s = re.sub(r"_Z\w+", "SYM", s)
    s = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", s)
    return re.sub(r"\s+", " ", s)


def parse(path):
    """{mangled name: {"body": [...], "desc": [...], "n": instructions, resources}}"""
    lines = open(path).read().split("\n")
    funcs, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            k = re.match(r"^\s*\.amdhsa_kernel (\S+)", lines[i])
            if k:
                j = i + 1
                while ".end_amdhsa_kernel" not in lines[j]:
                    j += 1
                funcs[k.group(1)]["desc"] = [x for x in map(norm, lines[i + 1:j]) if x]
                i = j
            i += 1
            continue
        name, j = m.group(1), i + 1
        while not lines[j].strip().startswith(".Lfunc_end"):
            j += 1
        body = [x for x in map(norm, lines[i + 1:j]) if x]
        f = {"body": body, "desc": [], "n": sum(1 for x in body if not x.startswith(".") and not x.endswith(":"))}
        for k in range(j, min(j + 60, len(lines))):      # the resource comments behind the function
            for key, short in RES:
                r = re.match(r"^\s*; %s: (\d+)" % key, lines[k])
                if r and short not in f:
                    f[short] = r.group(1)
        funcs[name] = f
        i = j + 1
    return funcs


def main():
    args, aliases = [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--alias":
            aliases.append(next(it).split("="))
        else:
            args.append(a)
    if not args or len(args) % 2:
        sys.exit(__doc__)
    bad = 0
    print("%-80s %6s %9s  %s" % ("function", "instr", "identical", "VGPR AGPR LDS scratch  (old -> new)"))
    old, new = {}, {}      # one pool per build: a function may have moved to the other translation unit
    for old_path, new_path in zip(args[0::2], args[1::2]):
        old.update(parse(old_path))
        new.update(parse(new_path))
    dm = demangle(sorted(set(old) | set(new)))
    used = set()
    for name in sorted(old, key=lambda n: dm[n]):
        partner = name if name in new else None
        for a, b in aliases:
            if partner is None and (a in name or a in dm[name]):
                partner = next((n for n in new if b in n or b in dm[n]), None)
        short = label(dm[name])
        fo = old[name]
        res_o = " ".join(fo.get(s, "-") for _, s in RES)
        if partner is None:
            print("%-80s %6d %9s  %s -> (gone)" % (short, fo["n"], "MISSING", res_o))
            bad += 1
            continue
        used.add(partner)
        fn = new[partner]
        same = fo["body"] == fn["body"] and fo["desc"] == fn["desc"]
        bad += not same
        if partner != name:
            short += " -> " + label(dm[partner])
        print("%-80s %6d %9s  %s -> %s" % (short, fo["n"], "yes" if same else "NO", res_o, " ".join(fn.get(s, "-") for _, s in RES)))
    for name in sorted(set(new) - used, key=lambda n: dm[n]):
        print("%-80s %6d %9s  (new function)" % (label(dm[name]), new[name]["n"], "NEW"))
        bad += 1
    sys.exit(1 if bad else 0)


main()
