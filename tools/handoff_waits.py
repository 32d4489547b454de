#!/usr/bin/env python3
"""The vector-memory waits (s_waitcnt vmcnt(n)) of the band kernel's hand-off code, read from the compiler's assembly
(hipcc -S for gfx950: cross-compiles without a GPU), for the four builds of recon_band.hip.

The source marks regions of the step loops of FRONT and CHROMA with inert assembly comments (WV_MARK in wave.h:
"; @mark <wave>.<region>.begin" / ".end"):
  front.look      the first look at the granule requested a step ago     front.request   the request for the next one
  front.prefetch  the coefficient prefetch behind the hand-off            front.free      the wait for a free record buffer
  front.record    the record's LDS stores
  chroma.look / chroma.request  as in FRONT                               chroma.prefetch the coefficient / record prefetch
  chroma.settle   where the step's loads are waited for, in front of its stores
  chroma.stores   the step's hand-off and pixel-row stores
Per region: every vmcnt wait between its marks, in the order of the listing, with the vector-memory instructions of the
listing since the last vmcnt(0) in front of it (what can at most be outstanding there, along the listing), and the
vector-memory instructions of the region itself. A region's cold blocks (the poll, a band's first step), which the
compiler lays out behind the loop, are outside the marks by construction.
usage: tools/handoff_waits.py [src.hip] [-D...]     (tests/test_handoff_waits_static.py asserts on waits())"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dryv_amd", "csrc", "recon_band.hip")
BUILDS = {"ILb0ELb0": "<false,false>", "ILb1ELb0": "<true,false>", "ILb0ELb1": "<false,true>", "ILb1ELb1": "<true,true>"}
VMEM = re.compile(r"^\s*(global_(?:load|store|atomic)\w*|buffer_(?:load|store|atomic)\w*|flat_(?:load|store|atomic)\w*)\b")
WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
MARK = re.compile(r";\s*@mark\s+(\S+)\.(begin|end)\s*$")


def assembly(src=SRC, flags=()):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I%s/include" % ROOT,
                            "--cuda-device-only", "-S", "-o", out, src, *flags], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-3000:])
        return open(out).read().splitlines()


def waits(src=SRC, flags=()):
    """{build: {region: {"waits": [(n, vm instructions since the last vmcnt(0))...], "vmem": [mnemonic...]}}}"""
    res, build, region, since = {}, None, None, 0
    for line in assembly(src, flags):
        m = re.match(r"^_ZN4dryv11band_kernel(ILb[01]ELb[01])E\w*:", line)
        if m:
            build, region, since = res.setdefault(BUILDS[m.group(1)], {}), None, 0
            continue
        if build is None:
            continue
        if re.match(r"^\s*s_endpgm", line):
            build = None
            continue
        m = MARK.search(line)
        if m:
            if m.group(2) == "begin":
                region = build.setdefault(m.group(1), {"waits": [], "vmem": []})
            else:
                region = None
            continue
        m = WAIT.match(line)
        if m:
            n = int(m.group(1))
            if region is not None:
                region["waits"].append((n, since))
            if n == 0:
                since = 0
            continue
        m = VMEM.match(line)
        if m:
            since += 1
            if region is not None:
                region["vmem"].append(m.group(1))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    src = args.pop(0) if args and not args[0].startswith("-") else SRC
    for b, regions in waits(src, args).items():
        print("band_kernel%s" % b)
        for name in sorted(regions):
            r = regions[name]
            w = ", ".join("vmcnt(%d) [<= %d in flight]" % x for x in r["waits"]) or "none"
            print("  %-16s waits: %-40s vector memory: %s" % (name, w, " ".join(r["vmem"]) or "-"))
