"""The low-pass wave's loop (SDRG_LPF_LOOP_IL_ASM, csrc/ssb_lpf_asm.h, tools/gen/gen_lpf_asm.py) is rotated by one
quad: after a chunk's 16th output write the wave runs the first quad of the next chunk on registers and only then
waits for its stores and meets the barrier; that quad's write is the first thing after the barrier (its output slot
is still being read during this iteration).

Structure, in each of the three chunk-mod-3 bodies: between the 16th ds_write_b128 and the branch to the barrier lie
one or two complete 4-sample quads (a quad is 8 v_pk_mul_f32 and 16 v_add_f32, the adds taking v48, v50, v49, v51 in
that order), no ds_write_b128, and the v[52:53] state capture comes before the quad.

Behaviour: the macro is run, one lane, on a small model of the wave (registers, SGPRs, one LDS with the lgkmcnt queue)
against the plain float32 recurrence: nch + 9 barriers exactly, every chunk's outputs complete in its ring slot at its
barrier and intact for the three iterations its readers need them, no register used while an LDS read of it may be in
flight, no store in flight at a barrier, and the carried state that of the last sample."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "sdr-for-android-lib_amd", "csrc", "ssb_lpf_asm.h")
SLOT = 16 * 68 * 4


def _loop():
    text = open(HDR).read()
    body = re.search(r"#define SDRG_LPF_LOOP_IL_ASM \\\n((?:    \".*\\\n)+)", text).group(1)
    return [l.strip()[1:-5] for l in body.splitlines() if l.strip() != '""']


def _bodies(lines):
    """the three bodies: from L_r<r> to the next body's label (the last one to the label after its barrier branch)"""
    at = {r: lines.index(f"L_r{r}_%=:") for r in range(3)}
    end = {0: at[1], 1: at[2], 2: lines.index("L_last_%=:")}
    return [lines[at[r] + 1:end[r]] for r in range(3)]


@pytest.mark.parametrize("r", [0, 1, 2])
def test_run_ahead_quad_between_last_write_and_barrier(r):
    body = _bodies(_loop())[r]
    writes = [i for i, l in enumerate(body) if l.startswith("ds_write_b128")]
    assert len(writes) == 16
    to_bar = [i for i, l in enumerate(body) if l.split()[0] in ("s_branch", "s_call_b64") and l.endswith("L_bar_%=")]
    assert len(to_bar) == 1 and to_bar[0] > writes[15]
    tail = body[writes[15] + 1:to_bar[0]]
    assert not any(l.startswith("ds_write_b128") for l in tail)
    muls = [l for l in tail if l.startswith("v_pk_mul_f32")]
    adds = [l for l in tail if l.startswith("v_add_f32")]
    assert len(muls) in (8, 16) and len(adds) == 2 * len(muls), (len(muls), len(adds))  # whole quads of 4 samples
    for i in range(0, len(adds), 4):
        assert [a.split(", ")[-1] for a in adds[i:i + 4]] == ["v48", "v50", "v49", "v51"], adds[i:i + 4]
    # one output register per sample, consecutive, from the start of an aligned 4-register quad
    outs = [int(a.split()[1][1:-1]) for a in adds[::4]]
    assert outs == list(range(outs[0], outs[0] + len(outs))) and outs[0] % 4 == 0, outs
    capture = [i for i, l in enumerate(tail) if l.startswith("v_pk_mov_b32 v[52:53]")]
    assert len(capture) == 1 and capture[0] < tail.index(muls[0])
    # nothing but the quad's write and its paired read between the return from the barrier and the chain
    first_mul = next(i for i, l in enumerate(body) if l.startswith("v_pk_mul_f32"))
    assert [l.split()[0] for l in body[:first_mul]] == ["ds_write_b128", "ds_read_b128"], body[:first_mul]


class Wave:
    """One lane of the low-pass wave: runs the macro's lines up to each s_barrier."""

    def __init__(self, lines, lds, c1, c2, z, nit, nch, abase, ybase):
        self.lines, self.lds = lines, lds
        self.labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        self.v = np.zeros(64, np.float32)
        self.vi = {}                     # VGPRs holding integers (v54)
        self.s = {"nit": nit, "nch": nch, "abase": abase, "ybase": ybase}
        self.f2 = {"c1": c1, "c2": c2, "z": np.array(z, np.float32)}
        self.queue = []                  # LDS operations in flight, oldest first: ("r", regs, values) or ("w",)
        self.busy = set()                # registers with a read in flight
        self.pc, self.scc, self.done = 0, 0, False

    def sval(self, t):
        return self.s[t[2:-1]] if t.startswith("%[") else int(t, 0)

    def pair(self, t):
        if t.startswith("%["):
            return self.f2[t[2:-1]]
        a = int(t[2:t.index(":")])
        assert not {a, a + 1} & self.busy, (self.lines[self.pc], "reads a register with an LDS read in flight")
        return self.v[a:a + 2]

    def wait(self, n):
        while len(self.queue) > n:
            op = self.queue.pop(0)
            if op[0] == "r":
                self.v[op[1]:op[1] + 4] = op[2]
                self.busy -= set(range(op[1], op[1] + 4))

    def vwrite(self, reg, val):
        assert reg not in self.busy, (self.lines[self.pc], "writes a register with an LDS read in flight")
        self.v[reg] = val

    def run_to_barrier(self):
        while True:
            if self.pc == len(self.lines):
                assert not self.queue, "LDS operations in flight at the end of the block"
                self.done = True
                return
            l = self.lines[self.pc]
            self.pc += 1
            if l.endswith(":") or l.startswith(("s_nop", "s_mov_b64")):
                continue
            op, _, rest = l.partition(" ")
            a =[x.strip() for x in rest.split(",")]
            if op == "s_barrier":
                assert not any(q[0] == "w" for q in self.queue), "a store in flight at the barrier"
                return
            if op == "s_setpc_b64":
                self.pc = self.s["ret"]
            elif op == "s_call_b64":
                self.s["ret"], self.pc = self.pc, self.labels[a[1]]
            elif op == "s_branch":
                self.pc = self.labels[a[0]]
            elif op == "s_cbranch_scc1":
                if self.scc:
                    self.pc = self.labels[a[0]]
            elif op == "s_waitcnt":
                self.wait(int(re.fullmatch(r"lgkmcnt\((\d+)\)", rest).group(1)))
            elif op == "s_mov_b32":
                self.s[a[0][2:-1]] = self.sval(a[1])
            elif op in ("s_add_i32", "s_sub_u32", "s_and_b32", "s_mul_i32"):
                x, y = self.sval(a[1]), self.sval(a[2])
                self.s[a[0][2:-1]] = {"s_add_i32": x + y, "s_sub_u32": x - y, "s_and_b32": x & y, "s_mul_i32": x * y}[op]
            elif op in ("s_cmp_le_i32", "s_cmp_ge_i32"):
                x, y = self.sval(a[0]), self.sval(a[1])
                self.scc = int(x <= y if op == "s_cmp_le_i32" else x >= y)
            elif op == "v_add_u32":
                self.vi[a[0]] = self.sval(a[1]) + self.sval(a[2])
            elif op == "v_pk_mov_b32":
                m = re.search(r"op_sel:\[(\d),(\d)\]", l)
                src0, src1 = re.findall(r"%\[\w+\]|v\[\d+:\d+\]", rest.split(" op_sel")[0])[1:3]
                lo, hi = self.pair(src0)[int(m.group(1))], self.pair(src1)[int(m.group(2))]
                if a[0].startswith("%["):
                    self.f2[a[0][2:-1]] = np.array([lo, hi], np.float32)
                else:
                    d = int(a[0][2:a[0].index(":")])
                    self.vwrite(d, lo)
                    self.vwrite(d + 1, hi)
            elif op == "v_pk_mul_f32":
                m = re.fullmatch(r"v\[(\d+):\d+\], (%\[c\d\]), (v\[\d+:\d+\]) op_sel:\[0,(\d)\] op_sel_hi:\[1,(\d)\]", rest)
                assert m and m.group(4) == m.group(5), l
                c, zv = self.pair(m.group(2)), self.pair(m.group(3))[int(m.group(4))]
                d = int(m.group(1))
                self.vwrite(d, c[0] * zv)
                self.vwrite(d + 1, c[1] * zv)
            elif op == "v_add_f32":
                d, x, y = (int(t[1:]) for t in a)
                assert not {x, y} & self.busy, (l, "reads a register with an LDS read in flight")
                self.vwrite(d, self.v[x] + self.v[y])
            elif op == "ds_read_b128":
                d = int(a[0][2:a[0].index(":")])
                addr, off = a[1].split(" offset:")
                w = (self.sval(addr) + int(off)) // 4
                assert not set(range(d, d + 4)) & self.busy
                self.queue.append(("r", d, self.lds[w:w + 4].copy()))
                self.busy |= set(range(d, d + 4))
            elif op == "ds_write_b128":
                data, off = a[1].split(" offset:")
                d = int(data[2:data.index(":")])
                assert not set(range(d, d + 4)) & self.busy
                w = (self.vi[a[0]] + int(off)) // 4
                self.lds[w:w + 4] = self.v[d:d + 4]  # may land at once ...
                self.queue.append(("w",))            # ... and is known to have landed only after a wait
            else:
                raise AssertionError(f"unmodelled instruction: {l}")


def _reference(x, c1, c2, z):
    z1, z2 = np.float32(z[0]), np.float32(z[1])
    y = np.empty_like(x)
    for i, v in enumerate(x):
        p1, p2 = c1 * z1, c2 * z2
        y[i] = (((v + p1[0]) + p2[0]) + p1[1]) + p2[1]
        z2, z1 = z1, y[i]
    return y, (z1, z2)


@pytest.mark.parametrize("dc_late", [False, True])
@pytest.mark.parametrize("nch", [0, 1, 2, 3, 4, 7])
def test_loop_model_equals_the_recurrence(nch, dc_late):
    """dc_late: the DC wave's chunk of an iteration lands at the iteration's end instead of its start (the low-pass
    wave may read a slot only after the barrier that completes it)"""
    rng = np.random.default_rng(nch)
    c1, c2 = np.array([1.9, -0.9], np.float32), np.array([0.01, -0.005], np.float32)
    z = (np.float32(0.25), np.float32(-0.125))
    x = rng.standard_normal(64 * nch).astype(np.float32)
    want, zwant = _reference(x, c1, c2, z)
    lds = np.full(7 * SLOT // 4, np.nan, np.float32)  # a[3] then y[4], this lane's row at offset 0 of each slot
    nit = nch + 9
    w = Wave(_loop(), lds, c1, c2, z, nit, nch, 0, 3 * SLOT)
    yrow = lambda c: lds[(3 + c % 4) * SLOT // 4:][:64]

    def dc(it):  # the DC wave writes chunk it - 1 during iteration it
        c = it - 1
        if 0 <= c < nch:
            lds[(c % 3) * SLOT // 4:][:64] = x[64 * c:64 * c + 64]

    for it in range(nit):
        if not dc_late:
            dc(it)
        w.run_to_barrier()
        assert not w.done, f"the block ended after {it} barriers, not {nit}"
        if dc_late:
            dc(it)
        # chunk it - 3 is complete at this barrier; its readers use it in iterations it + 1 (desired level) .. it + 3
        # (clamp), so chunks it - 3 .. it - 6 are intact now
        for c in range(it - 6, it - 2):
            if 0 <= c < nch:
                assert yrow(c).tobytes() == want[64 * c:64 * c + 64].tobytes(), (it, c)
    w.run_to_barrier()
    assert w.done, f"more than {nit} barriers"
    assert (w.f2["z"][0], w.f2["z"][1]) == (zwant if nch else z)
