#!/usr/bin/env python3
"""What the compiler made of a kernel's main loop: compile one .hip file of csrc/ to gfx950 assembly with the Makefile's flags and
report, per kernel, on the loop that holds the most MFMAs -- instruction counts, and for every `s_waitcnt vmcnt` how many MFMAs
lie between the issue of the youngest load it retires and the wait (a prefetch that the scheduler sank to its use shows as 0-3),
and the same for every `s_waitcnt lgkmcnt` and the youngest and the oldest LDS read it retires.

usage: python tools/isa_loop_report.py [conv_wino.hip] [--filter SUBSTRING] [--asm FILE.s]

Only matrix (v_mfma), vector-memory, LDS (ds_) and s_waitcnt / s_barrier instructions are looked at, plus the branches that give the
loop its shape.  Loads are told apart by their buffer descriptor: the SGPR quad that most of the loop's buffer loads use is the
weights', any other the halo's; global / flat loads are counted as "other".  vmcnt retires in issue order, so a wait for N
outstanding retires everything but the N youngest; the loop is walked three times and the third pass is reported, so loads issued
in one iteration and retired in the next are seen.  LDS operations return in issue order too (lgkmcnt; a loop with scalar
memory loads, which do not, is not what this is for), reads and writes in one queue.  Registers, scratch and LDS come from the compiler's resource remarks
(tools/kres.py)."""
import argparse, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sd_animation_optical_flow_amd", "csrc")


def makefile_flags(stem):
    """hipcc and the flags the Makefile compiles stem.hip with (CXXFLAGS, plus what the file's own rule adds)."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M))
    hipcc = os.environ.get("HIPCC", var.get("HIPCC", "hipcc"))
    flags = var["CXXFLAGS"].replace("$(ARCH)", var.get("ARCH", "gfx950")).split()
    m = re.search(r"^" + re.escape(stem) + r"\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\)(.*?)-c ", text, re.M)
    if m:
        flags += m.group(1).split()
    return hipcc, flags


def compile_asm(src):
    """-> (assembly text, resource rows of kres.parse_remarks)"""
    hipcc, flags = makefile_flags(os.path.splitext(os.path.basename(src))[0])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", kres.REMARKS, src, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return open(out).read(), kres.parse_remarks(r.stderr)


def functions(asm):
    """{mangled kernel name: [(kind, text)]}, kind in label / ins, comments stripped"""
    fns, cur = {}, None
    pending = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    for line in asm.splitlines():
        s = line.split(";")[0].rstrip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", s)
        if m:
            if m.group(1) in pending:
                cur = fns.setdefault(m.group(1), [])
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                cur.append(("label", m.group(1)))
            continue
        s = s.strip()
        if cur is not None and not s.startswith("."):
            cur.append(("ins", s))
    return fns


def branch_target(ins):
    m = re.match(r"s_c?branch\w*\s+(\S+)", ins)
    return m.group(1) if m else None


def loops(body):
    """Every backward branch is a loop: [(index of its target, index of the branch)]"""
    at = {t: i for i, (k, t) in enumerate(body) if k == "label"}
    return [(at[branch_target(t)], i) for i, (k, t) in enumerate(body)
            if k == "ins" and branch_target(t) in at and at[branch_target(t)] < i], at


def iteration(body, at, lo, hi):
    """The instructions of one trip round the loop [lo, hi] in execution order, from the block that is entered from outside.
    Forward conditional branches fall through (a skipped block is counted), the back edge and unconditional branches are taken."""
    header = lo
    for i, (k, t) in enumerate(body):
        if k == "ins" and not lo <= i <= hi and branch_target(t) in at and lo <= at[branch_target(t)] <= hi:
            header = at[branch_target(t)]
    seq, i = [], header
    for _ in range(4 * (hi - lo + 2)):
        k, t = body[i]
        nxt = i + 1
        if k == "ins":
            seq.append(t)
            tgt = branch_target(t)
            if tgt in at and lo <= at[tgt] <= hi and (i == hi or t.startswith("s_branch")):
                nxt = at[tgt]
        if nxt > hi:
            nxt = lo
        if nxt == header:
            return seq
        i = nxt
    raise RuntimeError("loop walk did not return to its header")


def is_mfma(t): return t.startswith("v_mfma") or t.startswith("v_smfma")
def is_vmem(t): return re.match(r"(buffer|global|flat|scratch)_(load|store|atomic)", t) is not None
def is_load(t): return re.match(r"(buffer|global|flat|scratch)_load", t) is not None


def analyse(seq):
    quads = {}
    for t in seq:
        m = re.match(r"buffer_load\w+\s+\S+\s*,\s*\S+\s*,\s*(s\[\d+:\d+\])", t)
        if m:
            quads[m.group(1)] = quads.get(m.group(1), 0) + 1
    wq = max(quads, key=quads.get) if quads else None

    def kind(t):
        if not is_load(t):
            return "store"
        if t.startswith("buffer_load"):
            return "weight" if wq and wq in t else "halo"
        return "other"

    rep = {"mfma": sum(map(is_mfma, seq)), "weight_loads": 0, "halo_loads": 0, "other_loads": 0,
           "lds_reads": sum(t.startswith("ds_read") or t.startswith("ds_load") for t in seq),
           "lds_writes": sum(t.startswith("ds_write") or t.startswith("ds_store") for t in seq),
           "barriers": sum(t.startswith("s_barrier") for t in seq), "waits": [], "lds_waits": [], "halo_store_wait": None}
    for t in seq:
        if is_load(t):
            rep[kind(t) + "_loads"] += 1

    fifo, mf, last_wait = [], 0, None   # outstanding vector-memory operations, oldest first: (kind, MFMAs issued before it)
    lfifo = []                          # ... and outstanding LDS operations: ("read" / "write", MFMAs issued before it)
    for trip in range(3):
        seen_write = False
        for t in seq:
            if is_mfma(t):
                mf += 1
            elif is_vmem(t):
                fifo.append((kind(t), mf))
            elif t.startswith("ds_write") or t.startswith("ds_store"):
                if trip == 2 and not seen_write and last_wait is not None:
                    rep["halo_store_wait"] = last_wait
                seen_write = True
                lfifo.append(("write", mf))
            elif t.startswith("ds_read") or t.startswith("ds_load"):
                lfifo.append(("read", mf))
            m = re.search(r"lgkmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
            if m:
                n = int(m.group(1))
                gone, lfifo = (lfifo[:len(lfifo) - n], lfifo[len(lfifo) - n:]) if len(lfifo) > n else ([], lfifo)
                reads = [g[1] for g in gone if g[0] == "read"]
                if trip == 2 and gone:
                    rep["lds_waits"].append({"lgkmcnt": n, "at_mfma": mf - base, "retired": len(gone), "reads": len(reads),
                                             "read_distance": mf - reads[-1] if reads else None,
                                             "oldest_read_distance": mf - reads[0] if reads else None})
            m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
            if m:
                n = int(m.group(1))
                last_wait = n
                gone, fifo = (fifo[:len(fifo) - n], fifo[len(fifo) - n:]) if len(fifo) > n else ([], fifo)
                if trip == 2:
                    w = {"vmcnt": n, "at_mfma": mf - base, "retired": len(gone)}
                    if gone:
                        w["youngest"] = gone[-1][0]
                        w["distance"] = mf - gone[-1][1]
                        wd = [mf - g[1] for g in gone if g[0] == "weight"]
                        w["weight_distance"] = min(wd) if wd else None
                    rep["waits"].append(w)
        base = mf
    wd = [w["weight_distance"] for w in rep["waits"] if w.get("weight_distance") is not None]
    rep["min_weight_distance"] = min(wd) if wd else None
    rd = [w["oldest_read_distance"] for w in rep["lds_waits"] if w["reads"]]
    rep["max_read_distance"] = max(rd) if rd else None
    return rep


def report(src=None, asm=None, name_filter=None):
    """-> [{kernel, mfma, weight_loads, halo_loads, other_loads, lds_reads, lds_writes, barriers, waits, lds_waits, halo_store_wait,
    min_weight_distance, max_read_distance, vgpr, agpr, scratch, lds}] for every kernel with a loop that holds MFMAs"""
    rows = []
    if asm is None:
        asm, rows = compile_asm(src)
    res = {r["name"]: r for r in rows}
    out = []
    for name, body in functions(asm).items():
        short = kres.short_name(name)
        if name_filter and name_filter not in short:
            continue
        ls, at = loops(body)
        best = None
        for lo, hi in ls:
            seq = iteration(body, at, lo, hi)
            n = sum(map(is_mfma, seq))
            if n and (best is None or (n, -(hi - lo)) > best[0]):
                best = ((n, -(hi - lo)), seq)
        if best is None:
            continue
        rep = analyse(best[1])
        r = res.get(name, {})
        rep.update(kernel=short, vgpr=r.get("VGPRs"), agpr=r.get("AGPRs"), scratch=r.get("ScratchSize"), lds=r.get("LDS"))
        out.append(rep)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src", nargs="?", default="conv_wino.hip", help="a file of csrc/ (or a path)")
    ap.add_argument("--filter", help="only kernels whose name contains this")
    ap.add_argument("--asm", help="analyse this assembly file instead of compiling (no register figures)")
    a = ap.parse_args()
    src = a.src if os.path.exists(a.src) else os.path.join(CSRC, a.src)
    reps = report(src, open(a.asm).read() if a.asm else None, a.filter)
    for r in reps:
        print(f"{r['kernel']}")
        print(f"  loop: {r['mfma']} MFMA, {r['weight_loads']} weight loads, {r['halo_loads']} halo loads, {r['other_loads']} other loads, "
              f"{r['lds_reads']} LDS reads, {r['lds_writes']} LDS writes, {r['barriers']} barriers")
        print(f"  vgpr {r['vgpr']} agpr {r['agpr']} scratch {r['scratch']} lds {r['lds']}")
        for w in r["waits"]:
            if w["retired"]:
                wd = "" if w["weight_distance"] is None else f", nearest weight load {w['weight_distance']} MFMAs"
                print(f"  after MFMA {w['at_mfma']:>3}: vmcnt({w['vmcnt']}) retires {w['retired']:>2}, youngest a {w['youngest']} load "
                      f"issued {w['distance']} MFMAs earlier{wd}")
            else:
                print(f"  after MFMA {w['at_mfma']:>3}: vmcnt({w['vmcnt']}) retires nothing")
        hw = r["halo_store_wait"]
        print(f"  last vmcnt wait before the loop's first LDS store: {'none' if hw is None else f'vmcnt({hw})'}")
        print(f"  weight loads: nearest wait {r['min_weight_distance']} MFMAs after issue")
        for w in r["lds_waits"]:
            what = (f"{w['reads']} reads, the youngest issued {w['read_distance']} MFMAs earlier, the oldest {w['oldest_read_distance']}"
                    if w["reads"] else "writes only")
            print(f"  after MFMA {w['at_mfma']:>3}: lgkmcnt({w['lgkmcnt']}) retires {w['retired']:>2} LDS operations: {what}")
        print(f"  LDS reads: farthest wait {r['max_read_distance']} MFMAs after issue")


if __name__ == "__main__":
    main()
