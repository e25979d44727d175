#!/usr/bin/env python3
"""Host model of K1Q's register-path step stream (deoss_amd/csrc/merkle_kernels.hpp).

Expands the DM_QS_* macros of the kernel header with the C preprocessor, interprets the
resulting instruction text on the 16 lanes of one DPP row (two leaves: e-quads on lanes 0..7,
a-quads 8 lanes up) and compares the chaining state after 1, 2, 3, 8, 9 and 2 x 8 linked blocks
with hashlib.sha256: a stream per ring stage (the compact kernel), and the stages of a run as ONE
stream with a link at every stage boundary, as the wide kernel sequences it ([8, 8],
[8, 8, 8, 8], [8, 8, 3]).  It also checks the DPP wait-state rule: no DPP source VGPR is written
by either of the two preceding instructions (the barrier between stages counts as none).
No GPU needed:  python tools/quad_stream_model.py
"""
import hashlib
import os
import re
import struct
import subprocess
import sys

HPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deoss_amd", "csrc", "merkle_kernels.hpp")
M = 0xFFFFFFFF
K256 = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M


def neg_kw(block):
    w = list(struct.unpack(">16I", block))
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & M)
    return [(-(K256[t] + w[t])) & M for t in range(64)]


def expand(names):
    """The instruction list of each macro in names, via cpp on the header's DM_QS_* defines."""
    src, keep = [], False
    for ln in open(HPP):
        if ln.startswith("#define DM_QS_"):
            keep = True
        if keep:
            src.append(ln)
            keep = ln.rstrip("\n").endswith("\\")
    src += ["@@MARK%d@@ %s\n" % (i, n) for i, n in enumerate(names)]
    out = subprocess.run(["cpp", "-P", "-"], input="".join(src), capture_output=True, text=True, check=True).stdout
    res = {}
    for i, n in enumerate(names):
        body = out.split("@@MARK%d@@" % i)[1].split("@@")[0]
        text = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', body)).replace("\\n", "\n").replace("\\t", " ")
        res[n] = [l.strip() for l in text.split("\n") if l.strip()]
    return res


def bitop3(a, b, c, tt):
    r = 0
    for i in range(8):
        if tt >> i & 1:
            t = (a if i & 4 else ~a) & (b if i & 2 else ~b) & (c if i & 1 else ~c)
            r |= t
    return r & M


class Row:
    """16 lanes; registers by operand name."""

    def __init__(self):
        self.v = {}
        self.recent = []   # destinations of the last two instructions
        self.count = 0

    def get(self, n):
        return self.v.setdefault(n, [0xDEAD0000 + i for i in range(16)])

    def run(self, insts):
        for ins in insts:
            if ins.startswith((".p2align", ".if", ".endif", "s_nop")):
                if ins.startswith("s_nop"):
                    self.recent = []
                continue
            self.count += 1
            op, rest = ins.split(None, 1)
            ops = re.findall(r"%\[(\w+)\]", rest)
            dst = ops[0]
            src = [list(self.get(o)) for o in ops[1:]]
            old = list(self.get(dst))
            banks = 0xF
            if op.endswith("_dpp"):
                assert ops[1] not in self.recent, "DPP wait states: %s" % ins
                m = re.search(r"bank_mask:0x([0-9a-f])", rest)
                banks = int(m.group(1), 16)
                qp = re.search(r"quad_perm:\[(\d),(\d),(\d),(\d)\]", rest)
                if qp:
                    perm = [int(x) for x in qp.groups()]
                    src[0] = [src[0][(i & ~3) + perm[i & 3]] for i in range(16)]
                else:
                    assert "row_ror:8" in rest, ins
                    src[0] = [src[0][(i - 8) % 16] for i in range(16)]
            if op == "v_alignbit_b32":
                new = [rotr(src[0][i], src[2][i]) for i in range(16)]
                assert ops[1] == ops[2]
            elif op == "v_bitop3_b32":
                tt = int(re.search(r"bitop3:0x([0-9a-f]+)", rest).group(1), 16)
                new = [bitop3(src[0][i], src[1][i], src[2][i], tt) for i in range(16)]
            elif op == "v_xor_b32_dpp":
                new = [src[0][i] ^ src[1][i] for i in range(16)]
            elif op == "v_sub_u32_dpp":
                new = [(src[0][i] - src[1][i]) & M for i in range(16)]
            elif op == "v_add_u32_dpp":
                new = [(src[0][i] + src[1][i]) & M for i in range(16)]
            elif op == "v_mov_b32_dpp":
                new = src[0]
            elif op == "v_add3_u32":
                new = [(src[0][i] + src[1][i] + src[2][i]) & M for i in range(16)]
            else:
                raise ValueError(ins)
            self.v[dst] = [new[i] if banks >> (i // 4) & 1 else old[i] for i in range(16)]
            self.recent = (self.recent + [dst])[-2:]


def load_k(row, prefix, kws):
    """kws[leaf] = the 64 words of a block; register q<t><w> of quad lane j = round 16t + 4j + w."""
    for t in range(4):
        for w in range(4):
            if prefix == "n" and (t > 0 or w > 2):
                continue
            name = "n%d" % w if prefix == "n" else "q%d%d" % (t, w)
            row.v[name] = [kws[(i >> 2) & 1][16 * t + 4 * (i & 3) + w] for i in range(16)]


def run_leaves(msgs, stages, code, one_stream=False):
    """msgs: two byte strings of equal whole-block length; stages: blocks per stage, in order.
    one_stream: the wide kernel's run of stages (quad_run_xstage): P = x and the fill at the first
    block of the first stage only, a DM_QS_LINKQ at every stage boundary (the next stage's block 0
    gives n0..n2), the drain at the last block of the last stage.  The barrier between two stages
    is no instruction: the DPP wait-state rule is checked straight across it."""
    if one_stream:
        stages = [sum(stages)]
    row = Row()
    # x: e-quads (e,f,g,h), a-quads (c,d,a,b); leaf l's e-quad = lanes 4l.., a-quad 8 up
    for k in range(4):
        row.v["x%d" % k] = [IV[(k + 2) & 3] if i >= 8 else IV[4 + k] for i in range(16)]
    row.v["sh"] = [((2, 13, 22, 0) if i >= 8 else (6, 11, 25, 0))[i & 3] for i in range(16)]
    row.v["msk"] = [0 if i >= 8 else M for i in range(16)]
    b = 0
    for n in stages:
        for k, nm in zip("abcd", range(4)):
            row.v[k] = list(row.v["x%d" % nm])   # P = x
        for i in range(n):
            load_k(row, "q", [neg_kw(m[64 * b:64 * b + 64]) for m in msgs])
            if i + 1 < n:
                load_k(row, "n", [neg_kw(m[64 * b + 64:64 * b + 128]) for m in msgs])
            head = "DM_QS_FILLQ" if i == 0 else "DM_QS_CONTQ"
            tail = "DM_QS_ENDLINKQ" if i + 1 < n else "DM_QS_ENDTAILQ"
            row.run(code[head] + code["DM_QS_BODYQ"] + code[tail])
            b += 1
    out = []
    for l in range(2):
        e = [row.v["x%d" % k][4 * l] for k in range(4)]
        a = [row.v["x%d" % ((k + 2) & 3)][8 + 4 * l] for k in range(4)]
        out.append(struct.pack(">8I", *(a + e)))
        # every lane of a quad's triple holds the same words
        for k in range(4):
            assert len({row.v["x%d" % k][4 * l + j] for j in range(3)}) == 1
            assert len({row.v["x%d" % k][8 + 4 * l + j] for j in range(3)}) == 1
    return out, row.count


def main():
    code = expand(["DM_QS_FILLQ", "DM_QS_CONTQ", "DM_QS_BODYQ", "DM_QS_ENDLINKQ", "DM_QS_ENDTAILQ"])
    for nm in ("DM_QS_FILLQ", "DM_QS_CONTQ", "DM_QS_BODYQ", "DM_QS_ENDLINKQ", "DM_QS_ENDTAILQ"):
        print("%-16s %4d instructions" % (nm, sum(1 for x in code[nm] if x.startswith("v_"))))
    ok = True
    for stages in ([1], [2], [3], [8], [9], [8, 8], [8, 3]):
        nb = sum(stages)
        msgs = [bytes((7 * i + 13 * l + nb) & 255 for i in range(64 * nb - 9)) for l in range(2)]
        padded = [m + b"\x80" + struct.pack(">Q", 8 * len(m)) for m in msgs]
        got, cnt = run_leaves(padded, stages, code)
        want = [hashlib.sha256(m).digest() for m in msgs]
        good = got == want
        ok &= good
        print("stages %-8s %5d instructions  %s" % (stages, cnt, "ok" if good else "MISMATCH"))
    # the wide kernel: the stages of a run as one stream, linked at every stage boundary
    for stages in ([8, 8], [8, 8, 8, 8], [8, 8, 3]):
        nb = sum(stages)
        msgs = [bytes((11 * i + 5 * l + nb) & 255 for i in range(64 * nb - 9)) for l in range(2)]
        padded = [m + b"\x80" + struct.pack(">Q", 8 * len(m)) for m in msgs]
        got, cnt = run_leaves(padded, stages, code, one_stream=True)
        _, per_stage = run_leaves(padded, stages, code)
        good = got == [hashlib.sha256(m).digest() for m in msgs]
        ok &= good
        print("run    %-14s %5d instructions (%d with a stream per stage)  %s" %
              (stages, cnt, per_stage, "ok" if good else "MISMATCH"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
