"""Static audit of the MFMA hazards around inline assembly.  hipcc pads the wait states between two
instructions it generated itself, but treats an `asm` statement as one opaque instruction: it neither pads inside the string
nor checks the statement's outputs against a matrix instruction still in flight (cdna_hip_programming.md §5.7 item 2).  A
violation gives wrong values on some waves of some launches and no message (round 6: the flow16 step's first layer).

This walks the device assembly of every kernel instantiation of the files that put vector instructions inside `asm`, block
by block, carrying the MFMAs in flight and the asm statements' recent writes across every control-flow edge (a branch
target receives the state of each predecessor, a loop head that of its back edge as well; iterated to a fixed point).
Only pairs with at least one side between `;;#ASMSTART` and `;;#ASMEND` are checked; the compiler pads the others.

  R1  WAR on SrcC: an asm instruction writes a register that an MFMA in flight reads as SrcC (C != D).
  R2  RAW / WAW on D: an asm instruction reads or writes an MFMA's D before its result is ready.
  R3  an asm VALU write, then an MFMA reading that register as A, B or C with fewer than 2 wait states in between
      (the compiler adds none after `;;#ASMEND` for a matrix instruction).

Wait states: one per instruction, N + 1 for `s_nop N`.  Required wait states per MFMA pass count (a pass = 4 cycles):
  R1 passes - 1                       CDNA3 ISA §7.6 "XDL read VGPR as SrcC, then VALU write" (2/4/8/16 passes: 1/3/7/15);
                                      LLVM GCNHazardRecognizer::checkMAIVALUHazards (…ReadVgprVALUWarWaitStates)
  R2 passes + 3, +1 on gfx950 past 2  CDNA3 ISA §7.6 "XDL write VGPR, then VALU read / write, VMEM / LDS read" (5/7/11/19);
                                      gfx950 adds one state (LLVM GFX940_XDL_N_PassWriteVgprVALUWawWaitStates): 5/8/12/20
  R3 2                                CDNA3 ISA §7.6 "VALU write VGPR, then MFMA read" (LLVM …VALUWritesVGPR…WaitStates)
Passes: MI355X issue cost (16x16x32 f16/bf16 16 cycles = 4 passes, 32x32x16 32 = 8, 32x32x2 f32 64 = 16, 16x16x4 f32
32 = 8); the f64 forms are taken as 16 passes (the strictest row) - where unsure, the stricter number.

usage: audit_asm_hazards.py [--jobs N] [extra hipcc flags]   compile the audited files to assembly and audit them
       audit_asm_hazards.py --asm FILE.s [FILE.s ...]         audit assembly a build already produced (csrc/Makefile)
       audit_asm_hazards.py --self-test FILE.s ...            audit hand-written snippets, print every finding, exit 0
Prints `N instantiations, M asm statements, K violations` and exits 1 on any violation."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aspire_amd", "csrc")
# the translation units whose kernels carry vector instructions inside asm statements (split2_f16 / split8_f16 / split4_range
# of asmc_flow_dev.h, through asmc_flow16_dev.h as well); tests/test_abi_and_layout.py checks that no other one does
SOURCES = ("asmc_flow16.hip", "asmc_flow.hip", "asmc_nsf.hip", "asmc_pcn_fused.hip")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-Wno-unused-function"]

PASSES = {"16x16x32": 4, "32x32x16": 8, "32x32x2": 16, "16x16x4": 8, "32x32x8": 8, "16x16x16": 4, "16x16x64": 4,
          "32x32x32": 8, "4x4x4": 2, "32x32x1": 16, "16x16x1": 8, "4x4x1": 2, "32x32x4": 16}
R3_NEED = 2


def mfma_passes(mn):
    if "_f64" in mn:
        return 16
    m = re.search(r"_(\d+x\d+x\d+)", mn)
    if not m or m.group(1) not in PASSES:
        raise ValueError(f"unknown matrix instruction {mn}: add its pass count to PASSES")
    return PASSES[m.group(1)]


def war_need(p):
    return p - 1


def raw_need(p):
    return p + 3 + (1 if p > 2 else 0)


REG = re.compile(r"(?<![\w.])([va])(?:\[(\d+):(\d+)\]|(\d+))(?![\w])")


def regs(text):
    out = set()
    for kind, lo, hi, one in REG.findall(text):
        if one:
            out.add((kind, int(one)))
        else:
            out.update((kind, r) for r in range(int(lo), int(hi) + 1))
    return frozenset(out)


def split_ops(rest):
    ops, depth, cur = [], 0, ""
    for ch in rest:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


class Ins:
    __slots__ = ("ln", "text", "mn", "asm", "stmt", "ws", "reads", "writes", "mfma", "target", "uncond", "end")

    def __init__(self, ln, text, asm, stmt):
        self.ln, self.text, self.asm, self.stmt = ln, text, asm, stmt
        parts = text.split(None, 1)
        self.mn = parts[0]
        ops = split_ops(parts[1]) if len(parts) > 1 else []
        self.reads, self.writes, self.mfma, self.target = frozenset(), frozenset(), None, None
        self.uncond = self.mn in ("s_branch", "s_setpc_b64")
        self.end = self.mn in ("s_endpgm", "s_setpc_b64", "s_trap", "s_endpgm_saved")
        m = re.fullmatch(r"s_nop\s+(0x[0-9a-fA-F]+|\d+)", text.strip())
        self.ws = int(m.group(1), 0) + 1 if m else 1
        if self.mn.startswith("s_branch") or self.mn.startswith("s_cbranch"):
            self.target = ops[0] if ops else None
            return
        if self.mn.startswith("v_mfma") or self.mn.startswith("v_smfmac"):
            d, a, b, c = (regs(o) for o in ops[:4])
            p = mfma_passes(self.mn)
            self.mfma = (d, a, b, c, p)
            self.reads, self.writes = a | b | c, d
            return
        if self.mn.startswith("v_"):
            if self.mn.startswith("v_swap"):
                self.writes = regs(ops[0]) | regs(ops[1])
                self.reads = self.writes
            elif ops:
                self.writes = regs(ops[0])
                self.reads = frozenset().union(*(regs(o) for o in ops[1:])) if len(ops) > 1 else frozenset()
                if self.mn.startswith("v_fma_mix") or "_sdwa" in self.mn or self.mn.startswith("v_writelane"):
                    self.reads = self.reads | self.writes  # partial writes keep the other half
            return
        if re.match(r"(ds|global|buffer|flat|scratch)_", self.mn):
            loads = re.search(r"load|read|_rtn", self.mn) or (("atomic" in self.mn) and re.search(r"\b(glc|sc0)\b", text))
            if loads and ops and not re.search(r"\blds\b", text):
                self.writes = regs(ops[0])
                self.reads = frozenset().union(*(regs(o) for o in ops[1:])) if len(ops) > 1 else frozenset()
            else:
                self.reads = frozenset().union(*(regs(o) for o in ops)) if ops else frozenset()


def functions(path):
    """yields (name, [Ins and ("label", name) entries]) per function of a device assembly file"""
    name, body, in_asm, stmt, pending = None, [], False, 0, set()
    for ln, line in enumerate(open(path), 1):
        t = line.strip()
        m = re.match(r"\.type\s+([\w.$]+),@function", t)
        if m:
            pending.add(m.group(1))
            continue
        if name is None:
            t = t.split(";", 1)[0].strip()
            if t.endswith(":") and t[:-1] in pending:
                name, body = t[:-1], []
            continue
        if t.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        if "#ASMSTART" in t:
            in_asm, stmt = True, stmt + 1
            continue
        if "#ASMEND" in t:
            in_asm = False
            continue
        t = t.split(";", 1)[0].strip()
        if not t:
            continue
        if re.fullmatch(r"[\w.$]+:", t):
            body.append(("label", t[:-1]))
            continue
        if t.startswith("."):
            continue
        body.append(Ins(ln, t, in_asm, stmt if in_asm else 0))
    if name is not None:
        yield name, body


def blocks(body):
    """basic blocks: (label or None, [Ins]) and the successor indices of each"""
    bl, cur = [], [None, []]
    for it in body:
        if isinstance(it, tuple):
            if cur[1] or cur[0] is not None:
                bl.append(cur)
            cur = [it[1], []]
            continue
        cur[1].append(it)
        if it.target is not None or it.end:
            bl.append(cur)
            cur = [None, []]
    if cur[1] or cur[0] is not None:
        bl.append(cur)
    index = {b[0]: i for i, b in enumerate(bl) if b[0] is not None}
    succ = []
    for i, (_, ins) in enumerate(bl):
        s = []
        last = ins[-1] if ins else None
        if last is not None and last.target is not None and last.target in index:
            s.append(index[last.target])
        if not (last is not None and (last.uncond or last.end)) and i + 1 < len(bl):
            s.append(i + 1)
        succ.append(s)
    return bl, succ


# the carried state: {item: fewest wait states since it issued, over every path}; items are
#   ("m", ln, asm, D, C, war, raw)   an MFMA (C: its SrcC registers that are not also D)
#   ("w", ln, regs)                   an asm instruction's VGPR write (R3)
def horizon(item):
    return max(item[5], item[6]) if item[0] == "m" else R3_NEED


def step(state, ins, report):
    for item, el in state.items():
        if item[0] == "m":
            _, pln, pasm, d, c, war, raw = item
            if not (pasm or ins.asm) or ins.mfma is not None:
                continue  # the compiler pads its own pairs; MFMA -> MFMA is outside this audit (no asm MFMAs: see below)
            if el < war and ins.writes & c:
                report("R1", pln, ins, el, war)
            if el < raw and (ins.writes | ins.reads) & d:
                report("R2", pln, ins, el, raw)
        elif ins.mfma is not None and el < R3_NEED and ins.reads & item[2]:
            report("R3", item[1], ins, el, R3_NEED)
    new = {}
    for item, el in state.items():
        e = el + ins.ws
        if e < horizon(item):
            new[item] = e
    if ins.mfma is not None:
        d, a, b, c, p = ins.mfma
        new[("m", ins.ln, ins.asm, d, c - d, war_need(p), raw_need(p))] = 0
    elif ins.asm and ins.mn.startswith("v_") and ins.writes:
        new[("w", ins.ln, ins.writes)] = 0
    return new


def join(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = min(v, out.get(k, v))
    return out


def audit_function(name, body, report):
    bl, succ = blocks(body)
    for _, ins in bl:
        for x in ins:
            if x.asm and x.mfma is not None:
                raise ValueError(f"{name}: matrix instruction inside asm (line {x.ln}): MFMA -> MFMA pairs are not audited")
    entry = [None] * len(bl)
    entry[0] = {} if bl else None
    work = list(range(len(bl)))
    quiet = lambda *a: None  # noqa: E731
    while work:  # fixed point of the entry states (min-join of wait states since issue; finite: everything ages out)
        i = work.pop(0)
        if entry[i] is None:
            continue
        st = entry[i]
        for x in bl[i][1]:
            st = step(st, x, quiet)
        for s in succ[i]:
            nxt = st if entry[s] is None else join(entry[s], st)
            if nxt != entry[s]:
                entry[s] = nxt
                if s not in work:
                    work.append(s)
    for i, (_, ins) in enumerate(bl):
        st = entry[i]
        if st is None:
            continue
        for x in ins:
            st = step(st, x, report)


def audit(paths, out=print):
    """audits assembly files; returns (instantiations, asm statements, [violation lines])"""
    n_fun, n_stmt, found = 0, 0, {}
    for path in paths:
        stmts = set()
        for name, body in functions(path):
            n_fun += 1
            stmts.update((x.stmt for x in body if not isinstance(x, tuple) and x.asm))

            def report(rule, pln, ins, el, need, name=name, path=path):
                key = (path, rule, pln, ins.ln)
                if key not in found:
                    found[key] = (f"{os.path.basename(path)}:{ins.ln} {rule} {el} of {need} wait states after line {pln}: "
                                  f"{ins.text}   [{name}]")

            audit_function(name, body, report)
        n_stmt += len(stmts)
    v = [found[k] for k in sorted(found)]
    for line in v:
        out(line)
    out(f"{n_fun} instantiations, {n_stmt} asm statements, {len(v)} violations")
    return n_fun, n_stmt, v


def compile_all(extra, jobs, outdir):
    def one(src):
        dst = os.path.join(outdir, src.replace(".hip", ".s"))
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", dst] + extra,
                       check=True, stderr=subprocess.DEVNULL)
        return dst

    with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16, len(SOURCES)))) as ex:
        return list(ex.map(one, SOURCES))


def main(argv):
    if argv[:1] == ["--self-test"]:
        audit(argv[1:])
        return 0
    if argv[:1] == ["--asm"]:
        n, s, v = audit(argv[1:])
        return 1 if v or not n else 0
    jobs = 16
    if argv[:1] == ["--jobs"]:
        jobs, argv = int(argv[1]), argv[2:]
    with tempfile.TemporaryDirectory(prefix="audit_hazards_") as tmp:
        paths = compile_all(argv, jobs, tmp)
        n, s, v = audit(paths)
    return 1 if v or not n else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
