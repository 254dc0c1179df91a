#!/usr/bin/env python3
"""Per-kernel comparison of two builds' gfx950 assembly (hipcc --cuda-device-only -S), without a GPU.

    python tools/isa_compare.py --old parent_encoder.s --new encoder.s encoder_train.s

For every kernel of the old files: registers, scratch, LDS and occupancy as the assembler comments give them, the counts of
v_mfma*, ds_read_b128 and buffer_load_dwordx4, whether the whole instruction stream is identical (labels renumbered), and whether
every K-loop block (a basic block that holds v_mfma and ends in a backward branch) has the same mnemonic sequence.
Exit status 1 if a kernel is missing, a K-loop block differs, or scratch / occupancy / LDS / an instruction count changed.

--mfma-blocks adds a column for kernels whose K loop spans several basic blocks (csrc/linear.hip: the chunk loop of k_linear_x3 /
k_linear_b16 is not one block, so the K-loop column reads "none" for them): the ordered mnemonic sequences of EVERY basic block that
holds a v_mfma, old against new; a difference is exit status 1 as well.

--sweep-blocks is for kernels that iterate on registers between workgroup barriers (csrc/stencil.hip: k_jacobi_band): for every kernel whose
stream differs it lists the basic blocks that hold an s_barrier, an LDS store and vector adds -- the sweep blocks -- with the counts of
v_add*, v_fma* / v_mul* / v_sub*, v_cndmask*, ds_read_b128 and ds_write_b128 in each, old against new, and the s_setprio of each; a
different number of such blocks or a different count (s_setprio aside) is exit status 1.
"""
import argparse, re, sys

META = {"vgpr": "NumVgprs", "sgpr": "TotalNumSgprs", "scratch": "ScratchSize", "occ": "Occupancy", "lds": "LDSByteSize"}
COUNTED = ("v_mfma", "ds_read_b128", "buffer_load_dwordx4")


def kernels(path):
    out, name, body = {}, None, []
    text = open(path).read().split("\n")
    kernel_names = {m.group(1) for l in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    for i, l in enumerate(text):
        m = re.match(r"^(\w+):", l)
        if m and m.group(1) in kernel_names:
            name, body = m.group(1), []
        elif name and l.startswith(".Lfunc_end"):
            meta = {}
            for c in text[i:i + 40]:
                for k, tag in META.items():
                    if (mm := re.match(r";\s*%s:\s*(\d+)" % tag, c)) and k not in meta:
                        meta[k] = int(mm.group(1))
            out[name] = (body, meta)
            name = None
        elif name is not None:
            l = re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip())
            if re.match(r"^\.LBB_\d+:", l) or (l.startswith("\t") and not l.lstrip().startswith(".")):
                if l.strip():
                    body.append(l.strip())
    return out


def mfma_blocks(body, loops_only):
    """Mnemonic sequences of the basic blocks that hold v_mfma, in order; loops_only: just those that end in a branch to their own or an
    earlier label."""
    blocks, seen, cur, label = [], {}, [], None
    for l in body + [".LBB_end:"]:
        if l.endswith(":"):
            blocks.append((label, cur))
            label, cur = l[:-1], []
            seen[label] = len(blocks)
        else:
            cur.append(l)
    res = []
    for idx, (label, ins) in enumerate(blocks):
        if not ins or not any(i.startswith("v_mfma") for i in ins):
            continue
        m = re.match(r"s_cbranch\w*\s+(\S+)", ins[-1]) or re.match(r"s_branch\s+(\S+)", ins[-1])
        if not loops_only or (m and m.group(1) in seen and seen[m.group(1)] <= idx):
            res.append([i.split()[0] for i in ins])
    return res


SWEEP_CLASSES = (("v_add",), ("v_fma", "v_mul", "v_sub"), ("v_cndmask",), ("ds_read_b128",), ("ds_write_b128",))


def sweep_blocks(body):
    """[(counts per SWEEP_CLASSES, number of s_setprio)] of the basic blocks that hold s_barrier, an LDS store and vector adds, in order"""
    blocks, cur = [], []
    for l in body + [".LBB_end:"]:
        if l.endswith(":"):
            blocks.append(cur)
            cur = []
        else:
            cur.append(l.split()[0])
    res = []
    for ins in blocks:
        if "s_barrier" in ins and any(i.startswith("ds_write") for i in ins) and any(i.startswith("v_add") for i in ins):
            res.append(([sum(i.startswith(c) for i in ins) for c in SWEEP_CLASSES], sum(i == "s_setprio" for i in ins)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--mfma-blocks", action="store_true", help="also compare every basic block that holds a v_mfma")
    ap.add_argument("--sweep-blocks", action="store_true", help="for kernels that differ: instruction-class counts of every sweep block")
    a = ap.parse_args()
    old, new = {}, {}
    for p in a.old:
        old.update(kernels(p))
    for p in a.new:
        new.update(kernels(p))
    bad = 0
    print("kernel | vgpr old/new | sgpr old/new | scratch | lds | occupancy | mfma ds_read_b128 buffer_load_x4 | instructions old/new | "
          "stream | K-loop blocks" + (" | MFMA blocks" if a.mfma_blocks else ""))
    for name in sorted(old):
        if name not in new:
            print(f"{name} | MISSING in new")
            bad += 1
            continue
        (bo, mo), (bn, mn) = old[name], new[name]
        co = [sum(i.startswith(c) for i in bo) for c in COUNTED]
        cn = [sum(i.startswith(c) for i in bn) for c in COUNTED]
        ko, kn = mfma_blocks(bo, True), mfma_blocks(bn, True)
        same = bo == bn
        kl = "none" if not ko and not kn else f"{len(ko)} {'same' if ko == kn else 'DIFFER'}"
        ok = all(mo.get(k) == mn.get(k) for k in ("scratch", "occ", "lds")) and co == cn and ko == kn
        if a.mfma_blocks:
            ao, an = mfma_blocks(bo, False), mfma_blocks(bn, False)
            nd = sum(x != y for x, y in zip(ao, an)) + abs(len(ao) - len(an))
            kl += " | " + ("none" if not ao and not an else f"{len(ao)} same" if not nd else f"{len(ao)}/{len(an)} {nd} DIFFER")
            ok = ok and not nd
        sweep_lines = []
        if a.sweep_blocks and not same:
            so, sn = sweep_blocks(bo), sweep_blocks(bn)
            ok = ok and [c for c, _ in so] == [c for c, _ in sn]
            sweep_lines.append(f"    sweep blocks {len(so)}/{len(sn)}: v_add | v_fma+v_mul+v_sub | v_cndmask | ds_read_b128 | ds_write_b128 (old/new), s_setprio")
            for i in range(max(len(so), len(sn))):
                co_, po = so[i] if i < len(so) else (None, None)
                cn_, pn = sn[i] if i < len(sn) else (None, None)
                sweep_lines.append(f"    block {i}: {co_} / {cn_} {'same' if co_ == cn_ else 'DIFFER'}, s_setprio {po}/{pn}")
        bad += not ok
        pair = lambda k: f"{mo.get(k)}/{mn.get(k)}" if mo.get(k) != mn.get(k) else f"{mo.get(k)}"
        print(f"{name} | {mo.get('vgpr')}/{mn.get('vgpr')} | {mo.get('sgpr')}/{mn.get('sgpr')} | {pair('scratch')} | {pair('lds')} | "
              f"{pair('occ')} | {' '.join(f'{x}' if x == y else f'{x}/{y}' for x, y in zip(co, cn))} | {len(bo)}/{len(bn)} | "
              f"{'identical' if same else 'differs'} | {kl}{'' if ok else ' | CHECK'}")
        for l in sweep_lines:
            print(l)
    for name in sorted(set(new) - set(old)):
        print(f"{name} | only in new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
