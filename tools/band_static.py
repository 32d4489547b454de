#!/usr/bin/env python3
"""Analysis only: instructions of band_kernel<false,false> between the phase marks of the source (-DDRYV_BAND_MARK turns
every PH(k) into an assembly comment), by class. Linear in the assembly: a section that the compiler laid out elsewhere
is counted where it landed. The classes go by opcode prefix alone:
  valu    v_*
  salu    s_* that is none of the next three
  branch  s_branch, s_cbranch_*, s_setpc / s_swappc / s_call
  wait    s_waitcnt*, s_nop
  misc    s_setprio, s_sleep, s_barrier, s_sendmsg*, s_sethalt, s_trap, s_icache_inv, s_endpgm ...
  lds     ds_*
  mem     everything else (global_*, buffer_*, flat_*)
Usage: tools/band_static.py [--roles] [extra -D flags]
  --roles  also prints one total per wave role over its step-loop sections alone (the sections of STEP_LOOP below)"""
import re, subprocess, sys, os, collections, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("valu", "salu", "branch", "wait", "misc", "lds", "mem")
BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")
WAIT = ("s_waitcnt", "s_nop")
MISC = ("s_setprio", "s_sleep", "s_barrier", "s_sendmsg", "s_sethalt", "s_trap", "s_icache_inv", "s_endpgm", "s_ttrace",
        "s_incperflevel", "s_decperflevel", "s_wakeup", "s_setkill", "s_code_end")
# The step loop of a role: the phase marks (PH's argument) of its function that OPEN a section of the loop (a section runs
# from its mark to the next one in the assembly).
STEP_LOOP = {
    "band_front": {"open": (0, 1, 2, 3), "what": "decode, residuals, hand-off, record"},
    "band_chroma": {"open": (0, 1, 2, 3), "what": "hand-off, residuals, prediction, lines + copies + flush"},
    "band_back": {"open": (0, 1, 2, 3, 4, 6, 5), "what": "edge arrays, chain, record freed, write-out + flush, step tail + wait"},
}


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "branch" if op.startswith(BRANCH) else "wait" if op.startswith(WAIT) else "misc" if op.startswith(MISC) else "salu"
    return "mem"


def main():
    args = sys.argv[1:]
    roles = "--roles" in args
    args = [a for a in args if a != "--roles"]
    out = os.path.join(tempfile.gettempdir(), "band_static.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-DDRYV_BAND_MARK", "-I%s/include" % root,
           "-S", "--cuda-device-only", "-o", out, "%s/dryv_amd/csrc/recon_band.hip" % root] + args
    subprocess.check_call(cmd)
    lines = open(out).read().split("\n")
    start = [i for i, l in enumerate(lines) if l.startswith(os.environ.get("BAND_SYM", "_ZN4dryv11band_kernelILb0ELb0E"))][0]
    end = [i for i, l in enumerate(lines) if i > start and "s_endpgm" in l][0]
    src = open("%s/dryv_amd/csrc/band_kernel.h" % root).read().split("\n")
    # the function a source line belongs to: the last "WV void band_xxx(" in front of it
    fn_at, fn = {}, "?"
    for n, l in enumerate(src, 1):
        m = re.match(r"WV void (band_\w+)\(", l)
        if m:
            fn = m.group(1)
        fn_at[n] = fn
    cur, cur_key = "prologue", None
    acc = collections.OrderedDict()
    keys = {}
    for l in lines[start:end]:
        m = re.search(r"; DRYV_MARK (\d+) (\d+)", l)
        if m:
            ln = int(m.group(1))
            cur = "after L%d %s" % (ln, src[ln - 1].strip()[:60])
            cur_key = (fn_at.get(ln, "?"), int(m.group(2)))
            continue
        t = l.strip()
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        acc.setdefault(cur, collections.Counter())[classify(t.split()[0])] += 1
        keys[cur] = cur_key
    fmt = "%5d valu %4d salu %4d branch %4d wait %3d misc %4d lds %3d mem   %s"
    for k, c in acc.items():
        print(fmt % tuple([c[x] for x in CLASSES] + [k]))
    if roles:
        print()
        for role, d in STEP_LOOP.items():
            tot = collections.Counter()
            for k, c in acc.items():
                if keys[k] and keys[k][0] == role and keys[k][1] in d["open"]:
                    tot.update(c)
            print(fmt % tuple([tot[x] for x in CLASSES] + ["%s step loop (%s): salu + branch = %d"
                                                           % (role, d["what"], tot["salu"] + tot["branch"])]))


if __name__ == "__main__":
    main()
