"""Branch coverage of the CPU oracle's path code (oracle/sail_oracle.cpp), measured with gcov. Test infrastructure only;
a helper module, not a conftest.

measure(cases) builds the oracle with -O0 --coverage and the project's FP flags into a temporary directory, renders
the cases in a child python whose SAIL_ORACLE_LIB points at that build (the mechanism tests/oracle.py has for the
sanitizer build), and parses `gcov -b -c --json-format`. It returns, for every conditional of the path code, how often
each outcome was taken in each case.

Scope. Path code is what a path runs: every function of sail_oracle.cpp defined above the `extern "C"` block (trace
and all it reaches, the primary-ray set-up included). oracle_render itself (argument checks, the accumulate modes, the
AOV stores), the display filters, oracle_pick / _math / _probe and the counters are out of scope; so is ref_math.h,
which tests/test_gpu_math_edges.py pins at its own branch and class edges.

Keys. An entry is (function, source text of the condition, outcome), never a line number. A condition is one operand
of a && / || chain, an if / while / for / ?: condition, or a case label of a switch; where a chain over class-typed
operands is first evaluated into a temporary, the chain as a whole is one more condition (gcc tests the temporary).
A condition that runs over several lines is read as one. A line whose conditions this module cannot tell apart is
keyed by its whole text and the arc's position (the gate asserts there is none).

What gcov invents. One rule: only arcs that gcov itself classes as `branch` and does not flag `throw` count. Its `call`
records (a call that might not return) are not branches, and the coverage build has -fno-exceptions, so no call grows
an exception edge.

Which arc is which outcome. gcov lists the two arcs of a conditional jump by destination block, so the first is the
one whose target gcc laid out first: the `then` side of an if / ?: / loop condition as written, `true` for an operand
of && that is not the last, `false` for an operand of || that is not the last, and for the last operand the side on
which the whole written condition (an outer ! included) is true. tests/test_oracle_branch_coverage.py checks these
rules against a small program with known counts before it believes any number."""
from __future__ import annotations

import json
import os
import pickle
import re
import shutil
import subprocess
import sys
import tempfile
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "oracle", "sail_oracle.cpp")
CXX = shutil.which(os.environ.get("CXX", "g++"))
GCOV = shutil.which("gcov")
AVAILABLE = CXX is not None and GCOV is not None
FLAGS = ["-O0", "--coverage", "-fno-exceptions", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
# the flush shim (our own text, built without coverage): one gcda per case instead of one per process
SHIM = 'extern "C" { void __gcov_dump(void); void __gcov_reset(void); void cov_flush(void) { __gcov_dump(); __gcov_reset(); } }\n'


# ---- building -------------------------------------------------------------------------------------------------------
def build(workdir: str, source: str = ORACLE_SRC, name: str = "sail_oracle", coverage: bool = True) -> str:
    """compile `source` into workdir/lib<name>.so; returns the library's path"""
    os.makedirs(workdir, exist_ok=True)
    lib = os.path.join(workdir, f"lib{name}.so")
    flags = [f for f in FLAGS if coverage or f != "--coverage"]
    args = [CXX, *flags, "-shared", "-I", os.path.dirname(ORACLE_SRC), source]
    if coverage:
        shim = os.path.join(workdir, "cov_flush.cpp")
        with open(shim, "w") as f:
            f.write(SHIM)
        subprocess.check_call([CXX, "-O0", "-fPIC", "-c", shim, "-o", shim[:-4] + ".o"], cwd=workdir)
        args.append(shim[:-4] + ".o")
    subprocess.check_call(args + ["-o", lib], cwd=workdir)
    return lib


# ---- the child: render cases with the library under SAIL_ORACLE_LIB --------------------------------------------------
def render_cases(lib: str, cases, outdir: str, flush: bool, timeout: int = 1200):
    """Render (id, scene, W, H, spp, bounces) cases in a child python against `lib`. Writes outdir/<i>.npz (accum, both
    AOV maps, segment count) and, with flush, outdir/<i>.gcda."""
    os.makedirs(outdir, exist_ok=True)
    job = os.path.join(outdir, "job.pkl")
    with open(job, "wb") as f:
        pickle.dump({"cases": list(cases), "outdir": outdir, "flush": flush, "lib": lib}, f)
    env = dict(os.environ, SAIL_ORACLE_LIB=lib)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", job], check=True, env=env, timeout=timeout,
                   cwd=ROOT)


def _child(job_path: str):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import glob

    import numpy as np

    import oracle
    from sail_amd import capi
    with open(job_path, "rb") as f:
        job = pickle.load(f)
    assert os.path.samefile(oracle.LIB, job["lib"])
    L = oracle.lib()
    libdir = os.path.dirname(job["lib"])
    if job["flush"]:
        L.cov_flush.restype = None
        L.cov_flush()  # drop what loading the library counted
        for g in glob.glob(os.path.join(libdir, "*.gcda")):
            os.remove(g)
    for i, (_, sc, w, h, spp, b) in enumerate(job["cases"]):
        inv, seeds = capi.schedule(np.array(sc["mvp_rowmajor"]), w, h, 0, spp)
        oracle.reset_counters()
        acc, an, ap = oracle.render(sc, capi.plugin_masks(sc["plugins"]), w, h, inv, seeds, sc["eye"], b, aov=True)
        segs, _ = oracle.counters()
        np.savez(os.path.join(job["outdir"], f"{i}.npz"), acc=acc, an=an, ap=ap, segs=np.int64(segs))
        if job["flush"]:
            L.cov_flush()
            (g,) = glob.glob(os.path.join(libdir, "*.gcda"))
            os.replace(g, os.path.join(job["outdir"], f"{i}.gcda"))


# ---- reading the source: which conditions a line holds --------------------------------------------------------------
def _strip_comment(line: str) -> str:
    return line.split("//", 1)[0].rstrip()


def _balanced(text: str, start: int) -> int:
    """index of the parenthesis that closes text[start] == '('"""
    depth = 0
    for i in range(start, len(text)):
        depth += text[i] == "("
        depth -= text[i] == ")"
        if depth == 0:
            return i
    raise ValueError(text)


def _top_level_split(text: str, op: str):
    parts, depth, last, i = [], 0, 0, 0
    while i < len(text):
        c = text[i]
        depth += c == "("
        depth -= c == ")"
        if depth == 0 and text.startswith(op, i):
            parts.append(text[last:i])
            last = i + len(op)
            i += len(op)
            continue
        i += 1
    parts.append(text[last:])
    return [p.strip() for p in parts]


def _unparen(text: str) -> str:
    text = text.strip()
    while text.startswith("(") and _balanced(text, 0) == len(text) - 1:
        text = text[1:-1].strip()
    return text


def _chain(text: str):
    """(operator or None, operands, negated) of a condition: a flat && or || chain, perhaps inside one outer !( )"""
    text, negated = _unparen(text), False
    if text.startswith("!") and text[1:].lstrip().startswith("(") and _balanced(text, text.index("(")) == len(text) - 1:
        inner = _unparen(text[1:])
        if len(_top_level_split(inner, "&&")) > 1 or len(_top_level_split(inner, "||")) > 1:
            text, negated = inner, True
    for op, other in (("&&", "||"), ("||", "&&")):
        parts = _top_level_split(text, op)
        if len(parts) > 1:
            flat = []
            for p in parts:
                p = _unparen(p)
                sub = _top_level_split(p, op)
                if len(_top_level_split(p, other)) > 1:
                    return None  # mixed operators: not told apart
                flat += [_unparen(s) for s in sub] if len(sub) > 1 else [p]
            return op, flat, negated
    return None, [text], negated


def _condition_spans(code: str):
    """the conditions of one line of code, in source order: [(position, text)]"""
    spans, taken = [], []
    for m in re.finditer(r"\b(if|while|for)\s*\(", code):
        open_ = m.end() - 1
        close = _balanced(code, open_)
        inner = code[open_ + 1:close]
        if m.group(1) == "for":
            clauses = inner.split(";")
            if len(clauses) != 3:
                continue
            inner = clauses[1]
        spans.append((open_, inner.strip()))
        taken.append((open_, close))
    depth_at = []
    depth = 0
    for c in code:
        depth_at.append(depth)
        depth += c == "("
        depth -= c == ")"
    for q in [i for i, c in enumerate(code) if c == "?"]:
        if any(a < q < b for a, b in taken):
            continue
        i, depth = q - 1, 0
        while i >= 0:
            c = code[i]
            if c == ")":
                depth += 1
            elif c == "(":
                if depth == 0:
                    break
                depth -= 1
            elif depth == 0:
                if c in ",;{:" or (c == "=" and code[i - 1] not in "=!<>" and code[i + 1] != "="):
                    break
                if code.startswith("return", i - 5) and i >= 5 and not (code[i - 6].isalnum() if i >= 6 else False):
                    break
            i -= 1
        spans.append((i + 1, code[i + 1:q].strip()))
        taken.append((i + 1, q))
    if not spans:  # a bool-valued chain: return A && B;  const bool x = A || B;
        m = re.search(r"(\breturn\b|[^=!<>]=(?!=))(.*);", code)
        if m:
            text = m.group(2).strip()
            op, _, _ = _chain(text) or (None, None, None)
            if op:
                spans.append((m.start(2), text))
    return sorted(spans)


def _switch_labels(lines, at: int):
    """case labels of the switch that opens on lines[at], in source order, `default` last"""
    depth, labels, started = 0, [], False
    for ln in lines[at:]:
        code = _strip_comment(ln)
        if not started:
            code = code[code.index("switch"):]
        for tok in re.finditer(r"\{|\}|\bcase\s+(\w+)\s*:|\bdefault\s*:", code):
            t = tok.group(0)
            if t == "{":
                depth += 1
                started = True
            elif t == "}":
                depth -= 1
                if started and depth == 0:
                    return labels
            elif depth == 1:
                labels.append("default" if t.startswith("default") else "case " + tok.group(1))
    return labels


def line_keys(lines, at: int, nbranches: int):
    """[(condition text, outcome)] for the nbranches arcs gcov lists on source line lines[at] (0-based)"""
    code, more = _strip_comment(lines[at]).strip(), at
    while code.count("(") > code.count(")") and more + 1 < len(lines) and more - at < 8:  # a condition over several lines
        more += 1
        code += " " + _strip_comment(lines[more]).strip()
    fallback = [(code, f"arc {i} of {nbranches}") for i in range(nbranches)]
    if re.search(r"\bswitch\s*\(", code):
        labels = _switch_labels(lines, at)
        if len(labels) == nbranches and labels[-1] == "default":
            return [("switch", lb) for lb in labels]
        return fallback
    if nbranches % 2:
        return fallback
    try:
        spans = _condition_spans(code)
        chains = [_chain(text) for _, text in spans]
    except (ValueError, IndexError):
        return fallback
    if not spans or any(c is None for c in chains):
        return fallback
    # a chain of several operands may come with one more jump on its temporary; find the one reading that fits
    sizes = [len(ops) for _, ops, _ in chains]
    base = sum(sizes)
    extra = nbranches // 2 - base
    multi = [i for i, s in enumerate(sizes) if s > 1]
    if extra == 0:
        with_tmp = set()
    elif extra == len(multi):
        with_tmp = set(multi)
    else:
        return fallback
    keys = []
    for i, ((_, text), (op, ops, negated)) in enumerate(zip(spans, chains)):
        for j, atom in enumerate(ops):
            last = j == len(ops) - 1
            if not last:
                first = "true" if op == "&&" else "false"
            elif i in with_tmp:
                first = "true"
            else:
                first = "false" if negated else "true"
            second = "false" if first == "true" else "true"
            keys += [(atom, first), (atom, second)]
        if i in with_tmp:
            whole = _unparen(text)
            first = "true"
            keys += [(whole, first), (whole, "false")]
    return keys if len(keys) == nbranches else fallback


# ---- reading gcov ---------------------------------------------------------------------------------------------------
def _gcov_json(workdir: str, gcno: str):
    out = subprocess.run([GCOV, "-b", "-c", "-m", "--json-format", "--stdout", gcno], cwd=workdir, check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out)


def parse(workdir: str, source: str, scope_end: int | None = None):
    """{(function, condition, outcome): count} of the gcda now in workdir, for the lines of `source` in scope"""
    src_base = os.path.splitext(os.path.basename(source))[0]
    (gcno,) = [f for f in os.listdir(workdir) if f.endswith(".gcno") and src_base in f]
    data = _gcov_json(workdir, gcno)
    with open(source) as f:
        lines = f.read().split("\n")
    if scope_end is None:
        scope_end = next((i + 1 for i, ln in enumerate(lines) if ln.startswith('extern "C"')), len(lines))
    counts = {}
    for fl in data["files"]:
        if os.path.basename(fl["file"]) != os.path.basename(source):
            continue
        names = {fn["name"]: fn["demangled_name"].split("(")[0].split("::")[-1] for fn in fl["functions"]}
        in_scope = {fn["name"] for fn in fl["functions"] if fn["start_line"] < scope_end}
        per_line, where = [], defaultdict(set)
        for ln in fl["lines"]:
            arcs = [b for b in ln["branches"] if not b["throw"]]
            if not arcs or ln["function_name"] not in in_scope:
                continue
            fn = names[ln["function_name"]]
            keys = line_keys(lines, ln["line_number"] - 1, len(arcs))
            per_line.append((ln["line_number"], fn, keys, arcs))
            for cond, _ in keys:
                where[(fn, cond)].add(ln["line_number"])
        for line_number, fn, keys, arcs in per_line:
            for (cond, outcome), arc in zip(keys, arcs):
                at = sorted(where[(fn, cond)])
                if len(at) > 1:  # the same text more than once in a function: told apart by order of appearance
                    cond = f"{cond}  [{at.index(line_number) + 1} of {len(at)}]"
                k = (fn, cond, outcome)
                counts[k] = counts.get(k, 0) + arc["count"]
    return counts


class Coverage:
    """per_case[key][case id] = count (non-zero entries only); keys holds every outcome of every conditional in scope"""

    def __init__(self):
        self.keys = set()
        self.per_case = defaultdict(dict)
        self.frames = {}

    def best(self, key, among=None):
        """(largest count within one single case, that case) over the cases `among` (default: all)"""
        d = self.per_case.get(key, {})
        if among is not None:
            d = {c: n for c, n in d.items() if c in among}
        if not d:
            return 0, None
        c = max(d, key=lambda c: d[c])
        return d[c], c

    def total(self, key, among=None):
        return sum(n for c, n in self.per_case.get(key, {}).items() if among is None or c in among)

    def report(self, among=None, need=8, unreachable=()):
        rows = []
        for k in sorted(self.keys):
            n, c = self.best(k, among)
            mark = "unreachable" if k in unreachable else ("ok" if n >= need else "MISSING")
            rows.append(f"{mark:11s} {k[0]:28s} {k[2]:14s} best {n:8d} in {str(c):34s} total {self.total(k, among):9d}  {k[1]}")
        return "\n".join(rows)


def measure(cases, source: str = ORACLE_SRC, workdir: str | None = None, keep_frames: bool = False) -> Coverage:
    """Coverage of `cases` = [(id, scene, W, H, spp, bounces)] (ids unique) on a coverage build of `source`."""
    import numpy as np
    cases = list(cases)
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    own = workdir is None
    workdir = workdir or tempfile.mkdtemp(prefix="sail_cov_")
    try:
        lib = build(workdir, source)
        out = os.path.join(workdir, "cases")
        render_cases(lib, cases, out, flush=True)
        cov = Coverage()
        src_base = os.path.splitext(os.path.basename(source))[0]
        (gcno,) = [f for f in os.listdir(workdir) if f.endswith(".gcno") and src_base in f]
        gcda = os.path.join(workdir, gcno[:-5] + ".gcda")
        for i, cid in enumerate(ids):
            os.replace(os.path.join(out, f"{i}.gcda"), gcda)
            for k, n in parse(workdir, source).items():
                cov.keys.add(k)
                if n:
                    cov.per_case[k][cid] = n
            if keep_frames:
                z = np.load(os.path.join(out, f"{i}.npz"))
                cov.frames[cid] = (z["acc"], z["an"], z["ap"], int(z["segs"]))
        return cov
    finally:
        if own:
            shutil.rmtree(workdir, ignore_errors=True)


def frames(cases, source: str = ORACLE_SRC, workdir: str | None = None):
    """{id: (accum, aov_n, aov_p, segments)} of `cases` on a plain -O0 build of `source` (no coverage): for mutants"""
    import numpy as np
    cases = list(cases)
    own = workdir is None
    workdir = workdir or tempfile.mkdtemp(prefix="sail_mut_")
    try:
        lib = build(workdir, source, coverage=False)
        out = os.path.join(workdir, "cases")
        render_cases(lib, cases, out, flush=False)
        res = {}
        for i, c in enumerate(cases):
            z = np.load(os.path.join(out, f"{i}.npz"))
            res[c[0]] = (z["acc"], z["an"], z["ap"], int(z["segs"]))
        return res
    finally:
        if own:
            shutil.rmtree(workdir, ignore_errors=True)


def write_report(path: str, need: int = 8):
    """the harness's report for the registry alone and for the registry plus the directed scenes (profiles/oracle_branch_coverage.txt)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import parity_cases
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "branch_scenes.json")) as f:
        scenes = json.load(f)
    with open(os.path.join(golden, "unreachable_branches.json")) as f:
        listed = {(e["function"], e["condition"], e["outcome"]): e["kind"] for e in json.load(f)}
    unreachable = {k for k, kind in listed.items() if kind == "unreachable"}
    reg = parity_cases.registry()
    directed = [("branch:" + n, s, s["W"], s["H"], s["spp"], s["bounces"]) for n, s in sorted(scenes.items())]
    cov = measure(reg + directed)
    reg_ids = {c[0] for c in reg}
    with open(path, "w") as f:
        for title, among in ((f"the registry alone ({len(reg)} frames: tests/parity_cases.py)", reg_ids),
                             (f"the registry plus the {len(directed)} directed scenes (tests/golden/branch_scenes.json)", None)):
            short = [k for k in cov.keys if cov.best(k, among)[0] < need]
            f.write(f"==== {title}\n{len(cov.keys)} outcomes of {len({k[:2] for k in cov.keys})} conditions in "
                    f"{len({k[0] for k in cov.keys})} functions; {len(short)} taken fewer than {need} times in every single frame, "
                    f"{len([k for k in short if k in unreachable])} of them on the unreachable list "
                    f"(tests/golden/unreachable_branches.json: {len(unreachable)} unreachable, {len(listed) - len(unreachable)} no_effect)\n")
            f.write(cov.report(among, need, unreachable) + "\n\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--report":
        write_report(sys.argv[2])
    else:
        sys.exit("usage: oracle_coverage.py --report OUT.txt   (--child JOB is started by measure())")
