#!/usr/bin/env python3
"""Mechanical validation of INTEGRATION.md against the reference tree, or against the index of it recorded in
tests/golden/reference_index.json (the tree does not travel with this repository). The Rust shim cannot be compiled here (no rustc), so this is what can be checked: every `path.rs:line[-line]` the
document cites must name a file that exists under the reference's src/ with those lines in range, and a Rust identifier
quoted in backticks or used in code on the same line as a citation must occur in that file (within a window around the
cited lines when it is not a declaration elsewhere in the file).
usage: tools/check_integration_refs.py [--index FILE | --write-index FILE] [doc ...]   (default: INTEGRATION.md)
exit status 1 on any finding. --index checks against a recorded index instead of the tree; --write-index checks against the
tree and records what the check needed of it: every source file's line count and the quoted identifiers it found there.
A document that cites a new line or quotes a new identifier needs the index written again, on a machine with the tree."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
CITE = re.compile(r"(?<![\w/.])((?:[\w]+/)*[\w]+\.rs):(\d+)(?:-(\d+))?(?:,\s*(\d+)-(\d+))?")
IDENT = re.compile(r"`([A-Za-z_][\w:.<>&\[\]; ]*?)(?:\(.*?\))?`")
# words in backticks that are not identifiers of the reference (this library's own names, Rust keywords, prose)
OWN = re.compile(r"^(dryv_|DRYV_|test_|Decoder(Error)?::Recon|i16|u8|u16|i8|isize|usize|todo!|\.take|Result|write_all|extern|frame_crop_|more_rbsp_data|README)")


def ref_files():
    out = {}
    for d, _, fs in os.walk(REF):
        for f in fs:
            if f.endswith(".rs"):
                p = os.path.join(d, f)
                out[os.path.relpath(p, REF)] = p
    return out


class Tree:
    """The reference's sources on disk."""
    def __init__(self):
        self.paths, self.texts, self.found = ref_files(), {}, set()
        self.files = list(self.paths)

    def text(self, rel):
        if rel not in self.texts:
            self.texts[rel] = open(self.paths[rel], errors="replace").read()
        return self.texts[rel]

    def n_lines(self, rel):
        return len(self.text(rel).splitlines())

    def has(self, word, rels=None):
        """Does `word` occur in one of the files `rels` (None: anywhere in the reference)?"""
        hit = any(word in self.text(r) for r in (self.files if rels is None else rels))
        if hit:
            self.found.add(word)
        return hit

    def index(self):
        return {"lines": {r: self.n_lines(r) for r in sorted(self.files)}, "identifiers": sorted(self.found)}


class Index:
    """What --write-index recorded of the tree. It does not know which file an identifier was found in: `has` answers for
    the whole reference, which is also what decides a finding against the tree."""
    def __init__(self, path):
        d = json.load(open(path))
        self.lines, self.words = d["lines"], set(d["identifiers"])
        self.files = list(self.lines)

    def n_lines(self, rel):
        return self.lines[rel]

    def has(self, word, rels=None):
        return word in self.words


def resolve(cite, files):
    """A citation names a path suffix ('frame/mod.rs', 'decoder.rs', 'pps.rs'): it must match exactly one file, or several
    of which exactly one lies on the decode path (src/video/...)."""
    cite = cite[4:] if cite.startswith("src/") else cite
    hits = [rel for rel in files if rel == cite or rel.endswith("/" + cite)]
    if len(hits) > 1:
        vid = [h for h in hits if h.startswith("video/")]
        if len(vid) == 1:
            hits = vid
    return hits


def check(doc, ref, idents):
    findings = []
    text = open(doc).read().splitlines()
    n_cites = 0
    for ln, line in enumerate(text, 1):
        cites = list(CITE.finditer(line))
        for m in cites:
            n_cites += 1
            hits = resolve(m.group(1), ref.files)
            if len(hits) != 1:
                findings.append("%s:%d: `%s` names %d files of the reference" % (doc, ln, m.group(1), len(hits)))
                continue
            n_src = ref.n_lines(hits[0])
            for a, b in ((m.group(2), m.group(3)), (m.group(4), m.group(5))):
                if a is None:
                    continue
                lo, hi = int(a), int(b or a)
                if not (1 <= lo <= hi <= n_src):
                    findings.append("%s:%d: %s:%d-%d is outside the file (%d lines)" % (doc, ln, hits[0], lo, hi, n_src))
        if cites and idents:
            # identifiers quoted on a line that cites the reference must occur in a file cited on this or a neighbouring
            # line -- or, failing that, somewhere in the reference (the document wraps its lines)
            near = []
            for l2 in text[max(0, ln - 2):ln + 1]:
                for m in CITE.finditer(l2):
                    h = resolve(m.group(1), ref.files)
                    if len(h) == 1:
                        near.append(h[0])
            for im in IDENT.finditer(line):
                name = im.group(1).strip()
                if OWN.match(name) or CITE.search(name) or "/" in name or " " in name or name.endswith(".md"):
                    continue
                last = re.sub(r"[^\w]", "", re.split(r"::|\.", name.strip("&"))[-1])
                if len(last) < 4 or ref.has(last, near):
                    continue
                if not ref.has(last):
                    findings.append("%s:%d: `%s` occurs nowhere in the reference" % (doc, ln, name))
    return n_cites, findings


def main(argv):
    index = write_index = None
    if argv[:1] == ["--index"]:
        index, argv = argv[1], argv[2:]
    elif argv[:1] == ["--write-index"]:
        write_index, argv = argv[1], argv[2:]
    docs = argv or [os.path.join(ROOT, "INTEGRATION.md")]
    if index is not None:
        ref = Index(index)
    elif os.path.isdir(REF):
        ref = Tree()
    else:
        print("reference tree absent: nothing to check")
        return 1 if write_index else 0
    bad = 0
    for d in docs:
        n, findings = check(d, ref, os.path.basename(d) == "INTEGRATION.md")
        print("%s: %d citations checked, %d findings" % (os.path.relpath(d, ROOT), n, len(findings)))
        for f in findings:
            print("  " + f)
        bad += len(findings)
    if write_index and not bad:
        with open(write_index, "w") as f:
            json.dump(ref.index(), f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
