"""numpy restatement of tidypopgen_amd/csrc/host/host_pwplan.h, the dealing of the pairwise kernels: nun units x S cuts of the K
range over W takers, full rounds decoded as before, what is left over in ONE more round cut into c pieces each.  Used by
tests/test_pwplan_host.py (against the header itself, compiled as a stand-alone program) and tests/test_gpu_pairwise_tail.py
(the plan a launch must have used)."""
import os
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_GROUPS = 8          # a piece of the tail keeps at least 8 groups of 128 loci
MAX_GROUPS = 131072     # 2^24 loci: the longest range one wave-unit may contract (FP32 accumulators of integer sums)

Plan = namedtuple("Plan", "nun S W kgs full L c total")


def make(nun, S, W, kgs, min_piece=MIN_GROUPS, cmax=0):
    full = nun * S // W * W
    L = nun * S - full
    c = 1
    if L:
        c = min(W // L, (kgs // S) // min_piece)
        if cmax > 0:
            c = min(c, cmax)
        c = max(c, 1)
    return Plan(nun, S, W, kgs, full, L, c, full + L * c)


def pieces(p):
    """(unit, k0, k1) of every index, as int64 arrays"""
    un = np.arange(p.total, dtype=np.int64)
    tail = un >= p.full
    t = np.where(tail, un - p.full, 0)
    sub = t // max(p.L, 1)
    u = np.where(tail, p.full + t - sub * p.L, un)
    cc = np.where(tail, p.c, 1)
    ks = u // p.nun
    lo, hi = p.kgs * ks // p.S, p.kgs * (ks + 1) // p.S
    return u - ks * p.nun, lo + (hi - lo) * sub // cc, lo + (hi - lo) * (sub + 1) // cc


def before(nun, S, kgs):
    """the decode the kernels had before there was a tail: index un < nun S is unit un % nun on cut un / nun"""
    un = np.arange(nun * S, dtype=np.int64)
    ks = un // nun
    return un % nun, kgs * ks // S, kgs * (ks + 1) // S


def cost(p, t_step, t_flush):
    c = (p.full // p.W) * (-(-p.kgs // p.S) * t_step + t_flush)
    if p.L:
        c += -(-p.kgs // (p.S * p.c)) * t_step + t_flush
    return c


def ksplit(nun, kgs, min_piece, minS, W, t_step, t_flush):
    cap = kgs // min_piece
    maxS = max(minS, min(cap, 96) if cap > 0 else 1)
    best, bestS = -1.0, minS
    for S in range(minS, maxS + 1):
        c = cost(make(nun, S, W, kgs, min_piece), t_step, t_flush)
        if best < 0 or c < best * 0.995:
            best, bestS = c, S
    return bestS


# ---- what the launchers of pairwise.hip hand to the plan ---------------------------------------------------------------------
ALL_T_STEP, ALL_T_FLUSH = 0.548, 10.1  # pw_launch_all's cost model: us per 128-locus group, us per flush


def units_all(n):
    """units (I, jt) of the five-product kernel: 96-row super-tiles I against 32-column tiles jt >= 3 I with data"""
    nct = -(-n // 32)
    return sum(jt // 3 + 1 for jt in range(nct))


def units_set(n, RA, RB):
    """units (I, J) of a (32 RA) x (32 RB) tile that hold a tile on or above the diagonal (pw_order_for)"""
    nct = -(-n // 32)
    nrg, ncg = -(-nct // RA), -(-nct // RB)
    return sum(1 for I in range(nrg) for J in range(ncg) if RB * J + RB - 1 >= RA * I)


def launch_plan(nun, m, num_cu=256, per_wg=4, ksteps=1, t_step=ALL_T_STEP, t_flush=ALL_T_FLUSH, S=0, cmax=0, nblk=0):
    """the plan of one launch over m < 2^27 loci: S, cmax, nblk as TPG_PW_PLAN forces them (0: not forced)"""
    kgs = -(-m // 128)
    assert kgs <= 8 * MAX_GROUPS
    W = per_wg * (nblk or max(num_cu // 8 * 8, 8))
    if not S:
        S = ksplit(nun, ksteps * kgs, MIN_GROUPS * ksteps, -(-kgs // MAX_GROUPS), W, t_step, t_flush)
    return make(nun, S, W, ksteps * kgs, MIN_GROUPS * ksteps, cmax)


def debug_line(p):
    """the tail of the library's TPG_DEBUG line for plan p"""
    return f"{p.nun} units, S = {p.S}, {p.full // p.W} full rounds of {p.W}, tail {p.L} x {p.c}"


def build_host_program(exe, sanitize=True):
    """tests/host/pwplan_main.cpp (csrc/host/host_pwplan.h on the host) -> exe"""
    san = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", *san, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
           "-I" + os.path.join(ROOT, "tidypopgen_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pwplan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host_program(exe, tmp, lines):
    """the queries of pwplan_main.cpp -> one (head, rows) per query: head the eight int32, rows a (total, 3) int32 array or None"""
    q, o = os.path.join(str(tmp), "pwplan_q.txt"), os.path.join(str(tmp), "pwplan_out.bin")
    with open(q, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, q, o], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    buf = np.fromfile(o, dtype=np.int32)
    out, at = [], 0
    for line in lines:
        head = buf[at:at + 8]
        at += 8
        if line.startswith("plan"):
            n = int(head[7]) * 3
            out.append((head, buf[at:at + n].reshape(-1, 3)))
            at += n
        else:
            out.append((head, None))
    assert at == buf.size
    return out
