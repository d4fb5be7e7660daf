"""Cut one kernel out of a hipcc -S --cuda-device-only listing and summarise it: instruction counts by kind, spills,
and (optionally) the longest loop bodies.  Usage: python tools/isa_extract.py file.s <substring of the mangled name> [out.s]

Compare two listings (or two directories of *.s with equal file names), e.g. before and after a change to a shared header:
    python tools/isa_extract.py diff old.s new.s [--rename OLD=NEW ...] [--pair OLD=NEW ...] [--only TEXT]
Kernels are paired by demangled name without namespace qualifiers (--rename maps a piece of a name of the old listing that
the change renamed, e.g. 'kernel<=kernel<HalfT, ' for a template that gained a parameter; --only keeps the kernels of
either listing whose name, after renaming, contains TEXT -- one element type of a listing that holds two); of each pair the instruction text is compared after dropping labels, directives, comments and symbol
names, and the .amdhsa_ resource block (registers, LDS, scratch).  One line per kernel: `identical`, `same instructions,
different order`, or `different` with counts; the exit status is 1 if any kernel is different or unpaired.

--pair OLD=NEW pairs kernels whose names no --rename can turn into one another: a kernel of the old listing whose name
contains OLD with the kernel of the new listing whose name contains NEW.  The name is the mangled one, or the demangled one
before its parameter list; `{}` stands for any text and must be the same text on both sides.  A side may be several
listings joined with `+`, for kernels that moved between files.  The tracker's five kernels against the one template
that replaced them (profiles/r28_track_unify.txt):
    python tools/isa_extract.py diff old/track.s+old/track_assign.s new/track.s \\
        --pair 'track_update_kernel<{}>=track_kernel<false, 0, false, {}>' \\
        --pair 'track_update2_kernel<{}>=track_kernel<true, 0, false, {}, int>' \\
        --pair 'track_update3_kernel<{}>=track_kernel<true, 1, false, {}, int, float const* restrict>' \\
        --pair 'track_update4_kernel<{}>=track_kernel<true, 2, false, {}, int, float const* restrict>' \\
        --pair 'track_update5_kernel<{}>=track_kernel<true, 2, true, {}, int, float const* restrict, App>'
"""
import collections
import os
import re
import subprocess
import sys


def kernels(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            if name:
                out[name] = buf
            name, buf = m.group(1), []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            if name:
                out[name] = buf
                name, buf = None, []
        if name:
            buf.append(line)
    return out


def resources(path):
    """mangled name -> the .amdhsa_ lines of the kernel's descriptor"""
    out, name = {}, None
    for line in open(path):
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            name = s.split()[1]
            out[name] = []
        elif s.startswith(".end_amdhsa_kernel"):
            name = None
        elif name:
            out[name].append(_no_symbols(s))
    return out


def _no_symbols(s):
    s = re.sub(r"\b(_Z\w+|__hip_cuid_\w+)", "SYM", s)
    return re.sub(r"\.L(BB|JTI|tmp|func_\w+?)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), s)


def instructions(body):
    out = []
    for line in body[1:]:
        s = line.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(_no_symbols(" ".join(s.split())))
    return out


def demangled(names):
    """(_Float16 goes in as the encoding of `half`, a builtin type like it: a demangler that does not know DF16_ would
    leave the whole name mangled; the result says _Float16 again)"""
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(n.replace("DF16_", "Dh") for n in names) + "\n",
                                 stdout=subprocess.PIPE, text=True, check=True)
            return [re.sub(r"\bhalf\b", "_Float16", n) for n in res.stdout.split("\n")[:len(names)]]
        except (OSError, subprocess.CalledProcessError):
            continue
    sys.exit("no demangler found (llvm-cxxfilt or c++filt)")


def _paired(mangled, plain, pairs, side):
    """--pair OLD=NEW: a kernel of the old listing (side 0) whose mangled name, or demangled name before the parameter
    list, contains OLD and one of the new listing (side 1) that contains NEW go under one name, NEW; every `{}` stands for
    any text, which must be the same on both sides ('update3_kernel<{}>=kernel<true, 1, {}, int>': one option per form)"""
    for pair in pairs:
        pattern = "(.+?)".join(re.escape(piece) for piece in pair[side].split("{}"))
        m = re.search(pattern, mangled) or re.search(pattern, plain.split("(")[0])
        if m:
            return pair[1].format(*m.groups())
    return plain


def by_plain_name(paths, renames, pairs=(), side=0):
    out = {}
    for path in paths.split("+"):
        ks, res = kernels(path), resources(path)
        for mangled, plain in zip(ks, demangled(list(ks))):
            plain = re.sub(r"(\(anonymous namespace\)|\b\w+)::", "", plain)
            for old, new in renames:
                plain = re.sub(r"\b%s\b" % re.escape(old), new, plain)
            plain = _paired(mangled, plain, pairs, side)
            assert plain not in out, plain
            out[plain] = (instructions(ks[mangled]), res.get(mangled))
    return out


def diff_listings(old, new, renames, only="", pairs=()):
    a, b = ({k: v for k, v in by_plain_name(path, rn, pairs, side).items() if only in k}
            for side, (path, rn) in enumerate(((old, renames), (new, []))))
    bad = 0
    for name in sorted(set(a) | set(b)):
        short = name if len(name) <= 150 else name[:147] + "..."
        if name not in a or name not in b:
            print(f"  {'only in new' if name in b else 'only in old'}: {short}")
            bad += 1
            continue
        (ia, ra), (ib, rb) = a[name], b[name]
        ca, cb = collections.Counter(ia), collections.Counter(ib)
        if ia == ib and ra == rb:
            verdict = "identical"
        elif ca == cb and ra == rb:
            moved = sum(x != y for x, y in zip(ia, ib))
            verdict = f"same instructions, different order ({moved} of {len(ia)} positions; registers, LDS, scratch equal)"
        else:
            gone, came = sum((ca - cb).values()), sum((cb - ca).values())
            verdict = f"different: {len(ia)} -> {len(ib)} instructions, {gone} only in old, {came} only in new"
            if ra != rb:
                verdict += "; resources: " + ", ".join(f"{x} -> {y}" for x, y in zip(ra or [], rb or []) if x != y)
            bad += 1
        print(f"  {verdict}: {short}")
    return len(set(a) | set(b)), bad


def diff_main(argv):
    renames = [tuple(argv[i + 1].split("=")) for i, x in enumerate(argv) if x == "--rename"]
    pairs = [tuple(argv[i + 1].split("=")) for i, x in enumerate(argv) if x == "--pair"]
    only = "".join(argv[i + 1] for i, x in enumerate(argv) if x == "--only")
    flags = ("--rename", "--pair", "--only")
    old, new = [x for i, x in enumerate(argv) if x not in flags and (i == 0 or argv[i - 1] not in flags)]
    if os.path.isdir(old):
        files = [(os.path.join(old, f), os.path.join(new, f)) for f in sorted(os.listdir(old)) if f.endswith(".s")]
    else:
        files = [(old, new)]
    total = bad = 0
    for o, n in files:
        print(" + ".join(os.path.basename(p) for p in o.split("+")), "->", " + ".join(os.path.basename(p) for p in n.split("+")))
        t, b = diff_listings(o, n, renames, only, pairs)
        total, bad = total + t, bad + b
    print(f"{total} kernels and device functions in {len(files)} listing(s): {bad} different or unpaired")
    return 1 if bad else 0


def main():
    if sys.argv[1] == "diff":
        sys.exit(diff_main(sys.argv[2:]))
    ks = kernels(sys.argv[1])
    key = sys.argv[2]
    for n, body in ks.items():
        if key not in n:
            continue
        text = "".join(body)
        cnt = lambda pat: len(re.findall(pat, text))
        print(n)
        print(f"  lines {len(body)}  mfma {cnt(r'v_mfma')}  ds_read {cnt(r'ds_read')}  ds_write {cnt(r'ds_write')}  "
              f"lds_dma {cnt(r'global_load_lds')}  scratch_st {cnt(r'scratch_store')}  scratch_ld {cnt(r'scratch_load')}  "
              f"accvgpr_rd {cnt(r'v_accvgpr_read')}  accvgpr_wr {cnt(r'v_accvgpr_write')}  v_mov {cnt(r'v_mov_b32')}  "
              f"s_waitcnt {cnt(r's_waitcnt')}  s_barrier {cnt(r's_barrier')}  s_nop {cnt(r's_nop')}")
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(text)


if __name__ == "__main__":
    main()
