#!/usr/bin/env python3
"""Registers, scratch and code size of every kernel of libcaenv.so, read from the compiler's own metadata.

  python tools/kernel_resources.py [--check] [--filter SUBSTR] [--against OTHER.s [--rename OLD=NEW ...]] [extra hipcc flags ...]

Compiles collision_avoidance_amd/csrc/ca_env.hip for gfx950 with the product flags plus -save-temps into build/isa/
(hipcc cross-compiles without a GPU), parses the `amdhsa.kernels` metadata of the device assembly and prints one row
per kernel: VGPRs, SGPRs, scratch bytes per lane (`.private_segment_fixed_size`), spilled VGPRs / SGPRs, static LDS,
code bytes, vector-instruction count.  --check exits non-zero if a step / quad / observation kernel uses scratch: a
spill at the 128-VGPR limit turns into HBM traffic (round 1: 19 MB per launch) and must not come back silently
(tests/test_host_cpu.py runs this check when the assembly is already there).

--against OTHER.s: the before / after table of a change that must not move the code.  OTHER.s is the device assembly of another
tree (this tool's build/isa/*.s there, copied aside).  One row per function with both sets of figures (OTHER's first), and
`identical` where the instruction text is the same after normalisation: comments, blank lines and section directives dropped, local
labels numbered in order of appearance.  It counts and compares; --check then fails when a name is on one side only, when a
kernel's VGPRs, SGPRs, scratch, spilled VGPRs or static LDS differ, when a function whose text differs has more vector instructions
or code bytes than OTHER's, or when a hot kernel uses scratch (as without --against).

--rename OLD=NEW (with --against, repeatable): a function of OTHER.s whose name -- as the table prints it, with its parameter list --
matches the regular expression OLD as a whole is paired with this tree's function of the name NEW (groups of OLD as \\1, \\2, ...),
and the pair is compared like any other.  A function's own symbol inside its text is written as one placeholder on both sides.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import build as b  # noqa: E402

OUT = os.path.join(ROOT, "build", "isa")
ASM = os.path.join(OUT, "ca_env-hip-amdgcn-amd-amdhsa-gfx950.s")
TILED_ARGS = re.compile(r"\(ca::Tiled\w+<[^()]*>::type\)")   # the tiled kernels' argument block, named by their template arguments already
HOT = ("step_kernel", "quad_kernel", "pair_kernel", "obs_kernel")   # kernels that must not spill


def compile_asm(extra=()):
    os.makedirs(OUT, exist_ok=True)
    cmd = [b.hipcc()] + b.HIPCC_FLAGS + list(extra) + ["-save-temps", "-o", os.path.join(OUT, "libcaenv_isa.so"), b.SOURCES[0]]
    subprocess.check_call(cmd, cwd=OUT)
    with open(os.path.join(OUT, "src_sha"), "w") as f:
        f.write(b.source_sha())


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout
        return out.splitlines()
    except Exception:
        return list(names)


def parse(asm_path=ASM):
    """[{name, vgpr, sgpr, scratch, vgpr_spill, sgpr_spill, lds, code_bytes, valu}] from the assembly file."""
    text = open(asm_path).read()
    # per function: "<sym>:" ... "; codeLenInByte = N" (the compiler's trailer); vector instructions counted in between
    valu, size = {}, {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?); codeLenInByte = (\d+)", text, re.S | re.M):
        valu[m.group(1)] = len(re.findall(r"^\s+v_", m.group(2), re.M))
        size[m.group(1)] = int(m.group(3))
    rows = []
    meta = text[text.rindex("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", meta)[1:]:
        def g(key, default=0):
            mm = re.search(r"^    \.%s:\s+(\S+)" % key, blk, re.M)
            return mm.group(1) if mm else default
        sym = g("name", "?")
        rows.append(dict(sym=sym, vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")),
                         scratch=int(g("private_segment_fixed_size")), vgpr_spill=int(g("vgpr_spill_count")),
                         sgpr_spill=int(g("sgpr_spill_count")), lds=int(g("group_segment_fixed_size")),
                         code_bytes=size.get(sym, 0), valu=valu.get(sym, 0)))
    for r, n in zip(rows, demangle([r["sym"] for r in rows])):
        r["name"] = TILED_ARGS.sub("", n.replace("void ca::", "").replace("(ca::StepArgs)", "").replace("(ca::ObsArgs)", ""))
    return rows


def functions(asm_path):
    """{symbol: normalised instruction text} of every function of the assembly file: comments, blank lines and section directives
    dropped, white space collapsed, the function's own symbol replaced, local labels (.LBB<function>_<block>, .Ltmp<n>, ...) renamed
    in order of appearance."""
    text = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines, labels = [], {}
        for ln in m.group(2).splitlines():
            ln = " ".join(ln.split(";", 1)[0].split())
            if ln and not re.match(r"\.(text|section)\b", ln):   # (where the function lies -- a template's own section -- is not its text)
                lines.append(ln)
        body = "\n".join(lines)
        for lab in re.findall(r"\.L\w+", body):
            labels.setdefault(lab, ".L%d" % len(labels))
        body = body.replace(m.group(1), "<self>")   # (a renamed function differs in its own symbol and nothing else)
        out[m.group(1)] = re.sub(r"\.L\w+", lambda mm: labels[mm.group(0)], body)
    return out


def short(name):
    return TILED_ARGS.sub("", name.replace("void ca::", "").replace("(ca::StepArgs)", "").replace("(ca::ObsArgs)", "")).replace("ca::", "")


FIGS = ("vgpr", "sgpr", "scratch", "vgpr_spill", "lds")   # what decides occupancy and scratch traffic: must not move


def against(other, flt=None, renames=()):
    """Prints the before / after table; returns the number of rows that break the bars: a name on one side only, a figure of FIGS
    moved, or differing text with more vector instructions or code bytes than the other side's.  renames: [(OLD, NEW)] of --rename."""
    new_f, old_f = functions(ASM), functions(other)
    new_k = {r["sym"]: r for r in parse(ASM)}
    old_k = {r["sym"]: r for r in parse(other)}
    syms = sorted(set(new_f) | set(old_f))
    names = dict(zip(syms, (short(n) for n in demangle(syms))))
    by_name = {names[s]: s for s in new_f}
    for s in [s for s in old_f if s not in new_f]:   # the other side's functions under this tree's symbols
        to = next((by_name.get(re.fullmatch(pat, names[s]).expand(new)) for pat, new in renames if re.fullmatch(pat, names[s])), None)
        if to is not None and to not in old_f:
            old_f[to] = old_f.pop(s)
            if s in old_k: old_k[to] = old_k.pop(s)
            names[to] = "%s <- %s" % (names[to].split("(")[0], names[s].split("(")[0])   # (printed whole: label())
            syms.remove(s)
    size = lambda body: len(re.findall(r"^v_", body, re.M))
    label = lambda s: names[s] if " <- " in names[s] else names[s][:52]
    bad = same = 0
    print("%-52s %11s %11s %11s %9s %11s %15s %13s  %s" % ("function (other -> this)", "VGPR", "SGPR", "scratch", "v-spill", "LDS", "code B", "VALU", "text"))
    for s in sorted(syms, key=lambda s: names[s]):
        if flt and flt not in names[s]:
            continue
        if s not in new_f or s not in old_f:
            print("%-52s only in %s" % (names[s][:52], "this tree" if s in new_f else "the other"))
            bad += 1
            continue
        o, n = old_k.get(s), new_k.get(s)
        pair = lambda k, w: ("%d -> %d" % (o[k], n[k])).rjust(w) if o and n else "-".rjust(w)
        ident = new_f[s] == old_f[s]
        same += ident
        moved = bool(o and n) and any(o[k] != n[k] for k in FIGS)
        grew = not ident and (size(new_f[s]) > size(old_f[s]) or bool(o and n) and n["code_bytes"] > o["code_bytes"])
        bad += moved or grew
        valu = ("%d -> %d" % (size(old_f[s]), size(new_f[s]))).rjust(13)
        print("%-52s %s %s %s %s %s %s %s  %s" % (label(s), pair("vgpr", 11), pair("sgpr", 11), pair("scratch", 11), pair("vgpr_spill", 9),
                                                 pair("lds", 11), pair("code_bytes", 15), valu,
                                                 "identical" if ident else ("differs, FIGURES MOVED" if moved else ("differs, GREW" if grew else "differs"))))
    print("\n%d functions, %d with identical instruction text, %d differ; %d break a bar (a name on one side only; VGPRs / SGPRs / scratch / "
          "spilled VGPRs / static LDS moved; differing text with more vector instructions or code bytes)" % (len(syms), same, len(syms) - same, bad))
    return bad


def by_design(name):
    """The LDS-line-table variant step_kernel<K, BS, 0, SMX, ...> keeps LP3's projected lines in a private array (ca_lp.h lp3:
    only the few lanes whose LP2 is infeasible touch it); every other hot kernel must run without scratch memory."""
    # (Rounds 3-4 also exempted the K = 10 register-line kernels of two and more waves with obstacle lists of 16 -- two of their
    # 14 line slots lived in scratch -- and quad_kernel<10, 512, 16>.  Round 5: the register allocator took the two rare stages'
    # `while (true)` loops for hot and the fully unrolled LP2 for cold; with the loops marked unlikely and the rare stages' constants
    # and addresses formed where they are used, EVERY instantiation that pick_variant can select for K <= 10 has ScratchSize 0.)
    return re.match(r"step_kernel<\d+, \d+, 0, \d+(, \w+)*>", name) is not None


def spilling(rows):
    return [r for r in rows if any(h in r["name"] for h in HOT) and not by_design(r["name"]) and (r["scratch"] or r["vgpr_spill"])]


def ensure_asm(extra=()):
    fresh = os.path.exists(ASM) and os.path.exists(os.path.join(OUT, "src_sha")) and \
        open(os.path.join(OUT, "src_sha")).read() == b.source_sha() and not extra
    if not fresh:
        compile_asm(extra)


def main():
    args = sys.argv[1:]
    check = "--check" in args
    flt = None
    if "--filter" in args:
        flt = args[args.index("--filter") + 1]
    other = args[args.index("--against") + 1] if "--against" in args else None
    renames = [tuple(args[k + 1].split("=", 1)) for k, a in enumerate(args) if a == "--rename"]
    extra = [a for a in args if a.startswith("-") and a not in ("--check", "--filter", "--against", "--rename")]
    ensure_asm(extra)
    if other:
        bad = against(other, flt, renames)
        spills = spilling(parse())
        for r in spills:
            print("hot-path kernel with scratch memory: %s: %d B per lane, %d VGPRs spilled" % (r["name"], r["scratch"], r["vgpr_spill"]))
        if check and (bad or spills):
            raise SystemExit(1)
        return
    rows = parse()
    print("%-52s %5s %5s %8s %7s %7s %7s %9s %7s" % ("kernel", "VGPR", "SGPR", "scratch", "v-spill", "s-spill", "LDS", "code B", "VALU"))
    for r in sorted(rows, key=lambda r: r["name"]):
        if flt and flt not in r["name"]:
            continue
        print("%-52s %5d %5d %8d %7d %7d %7d %9d %7d" % (r["name"][:52], r["vgpr"], r["sgpr"], r["scratch"], r["vgpr_spill"],
                                                       r["sgpr_spill"], r["lds"], r["code_bytes"], r["valu"]))
    bad = spilling(rows)
    if bad:
        print("\nkernels of the hot path that use scratch memory:")
        for r in bad:
            print("   %s: %d B per lane, %d VGPRs spilled" % (r["name"], r["scratch"], r["vgpr_spill"]))
        if check:
            raise SystemExit(1)
    elif check:
        print("\nno hot-path kernel uses scratch memory")


if __name__ == "__main__":
    main()
