"""Per-basic-block VALU / SALU / LDS / VMEM instruction counts of one kernel in a device .s file.

    hipcc ... -DHMC_WAVE_PROD_ONLY --offload-device-only -S -o /tmp/wave.s hmc_wave.hip
    python scripts/dev/valu_blocks.py /tmp/wave.s 'k_wave_iters_k1ILb0ELb0ELb0ELb0ELb0ELb1E'

(the last template flag is TT: ...ELb1E the three-term leapfrog instance, ...ELb0E the two-FMA one)

A static view for A/B work on instruction counts (the PMC SQ_INSTS_VALU pass is the measurement).

With a price table as third argument (the output of scripts/ubench/instr_prices.hip, e.g.
profiles/rr_instr_prices.txt) a column of VALU issue slots is added: every VALU instruction weighted
with its opcode's cost relative to v_fma_f64 (the vs_fma column; opcodes the table does not list
count 1).
"""
import re
import sys


def kernel_lines(path, pat):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(pat) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def read_prices(path):
    prices = {}
    for l in open(path):
        f = l.split()
        if len(f) == 5 and f[0].startswith("v_"):
            prices[f[0]] = float(f[3])
    return prices


def price_of(op, prices):
    if op in prices:                                  # a form priced on its own (v_mov_b32_dpp)
        return prices[op]
    if op.endswith(("_dpp", "_sdwa")):                # no other DPP / SDWA form was priced
        return 1.0
    return prices.get(re.sub(r"_(e32|e64)$", "", op), 1.0)


def main():
    path, pat = sys.argv[1], sys.argv[2]
    prices = read_prices(sys.argv[3]) if len(sys.argv) > 3 else None
    blocks, cur = [], ["entry", 0, 0, 0, 0, "", 0.0]
    for l in kernel_lines(path, pat):
        s = l.strip()
        m = re.match(r"^(\.LBB\S+):(.*)$", s) or re.match(r"^; %(bb\.\d+):(.*)$", s)
        if m:
            blocks.append(cur)
            cur = [m.group(1), 0, 0, 0, 0, m.group(2).strip()[:60], 0.0]
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        if op.startswith("v_"):
            cur[1] += 1
            cur[6] += price_of(op, prices) if prices else 1.0
        elif op.startswith("s_") and op not in ("s_nop", "s_waitcnt"):
            cur[2] += 1
        elif op.startswith("ds_"):
            cur[3] += 1
        elif op.startswith(("global_", "buffer_", "scratch_")):
            cur[4] += 1
    blocks.append(cur)
    tot, slots = [0, 0, 0, 0], 0.0
    sl = f" {'slots':>7s}" if prices else ""
    print(f"{'block':14s} {'VALU':>5s} {'SALU':>5s} {'LDS':>4s} {'VMEM':>4s}{sl}  note")
    for b in blocks:
        sl = f" {b[6]:7.1f}" if prices else ""
        print(f"{b[0]:14s} {b[1]:5d} {b[2]:5d} {b[3]:4d} {b[4]:4d}{sl}  {b[5]}")
        for i in range(4):
            tot[i] += b[i + 1]
        slots += b[6]
    sl = f" {slots:7.1f}" if prices else ""
    print(f"{'total':14s} {tot[0]:5d} {tot[1]:5d} {tot[2]:4d} {tot[3]:4d}{sl}")


if __name__ == "__main__":
    main()
