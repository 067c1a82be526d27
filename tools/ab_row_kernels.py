"""The row kernels on csrc/row_pieces.h against a built checkout of the parent commit: output bits, code generation, speed.

  python tools/ab_row_kernels.py --parent-root DIR [--parts resources,bits,time] [--arms bench,decode,adamw,step] [--rounds 3]
                                 [--step-modes frozen,unfrozen] [--out profiles/row_pieces_ab.txt]

resources  (no GPU) elementwise.hip, decode.hip and kv8.hip of both trees compiled for gfx950 with -Rpass-analysis=kernel-resource-usage:
           VGPRs, SGPRs, scratch, LDS and occupancy per kernel instantiation, every instantiation of this tree checked against the one it
           replaces (no more scratch, no lower occupancy), and the ISA bodies of the host-scale AdamW kernels and of the bf16
           rmsnorm_fwd_kernel compared.
bits       seeded inputs from the CPU generator; one fresh child process per build runs every touched entry point in bf16 and fp32 and
           writes a SHA-256 of the raw bytes of every output array; the two lists must be identical.
time       both builds alternate, --rounds rounds each, one fresh process per arm: bench.py, tools/bench_decode.py, the AdamW table and
           the whole step of tools/bench_grad_clip.py.  The branch's median may exceed the parent's by no more than the parent's own
           spread (max - min over its rounds).
A part that needs a GPU and finds none fails; nothing here falls back.  The report goes to --out (sections of parts not run are kept from
the file that is there)."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("elementwise.hip", "decode.hip", "kv8.hip")


# ---------------------------------------------------------------------------------------------------------------- resources
def compile_remarks(root, tmp):
    """-> ({demangled kernel: {file, VGPRs, SGPRs, scratch, LDS, occupancy}}, {demangled kernel: ISA body lines})."""
    sys.path.insert(0, ROOT)
    from egoscaler_amd import build as B                               # the flags are this tree's for both: build.py has not changed
    res, isa = {}, {}
    for f in FILES:
        cmd = [B._hipcc(), *B.COMMON[:-2], "-I", os.path.join(root, "include"), *B.EXTRA.get(f, []), "--cuda-device-only", "--save-temps", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(root, "egoscaler_amd", "csrc", f),
               "-o", os.path.join(tmp, f + ".o")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise SystemExit(f"hipcc failed on {f} of {root}:\n{r.stderr[-4000:]}")
        cur = None
        for ln in r.stderr.splitlines():
            m = re.search(r"remark: .*?:\d+:\d+:\s+(.*?) \[-Rpass-analysis", ln)
            if not m:
                continue
            key, _, val = m.group(1).partition(": ")
            if key == "Function Name":
                cur = res.setdefault(val, {"file": f})
            elif cur is not None:
                name = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
                        "LDS Size [bytes/block]": "LDS"}.get(key.strip())
                if name:
                    cur[name] = int(val)
        asm = [p for p in os.listdir(tmp) if p.startswith(f[:-4] + "-hip-amdgcn") and p.endswith(".s")]
        body, name = None, None
        for ln in open(os.path.join(tmp, asm[0])):
            m = re.match(r"(_Z\w+):", ln)
            if m and m.group(1) in res:
                name, body = m.group(1), []
            elif body is not None:
                if ln.strip().startswith(".section"):                 # the kernel descriptor follows the code
                    isa[name], body = body, None
                elif ln.strip() and not ln.lstrip().startswith(";"):
                    body.append(ln.split(";")[0].strip())
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = {n: re.sub(r"^void |\(.*$", "", d) for n, d in zip(names, dem)}
    return {short[n]: v for n, v in res.items()}, {short[n]: v for n, v in isa.items()}


def replaced_by(parent_name):
    """The instantiation of this tree that does the work of the parent's `parent_name`."""
    n = re.sub(r"^(rmsnorm_fwd_tail_kernel|slabs_rmsnorm_kernel)<", "rmsnorm_slabs_kernel<", parent_name)
    m = re.match(r"adamw(_vec4)?(_ds)?_kernel<(.*)>$", n)
    if m:
        n = f"adamw{m.group(1) or ''}_kernel<{m.group(3)}, {'float const*' if m.group(2) else 'float'}>"
    return n


def isa_equal(a, b):
    """How far two ISA bodies agree (block labels carry the function's number and are renumbered first)."""
    def labels(body):
        return [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in body]

    def regs(body):
        return [re.sub(r"\b[vsa]\[\d+:\d+\]|\b[vsa]\d+\b", "R", ln) for ln in labels(body)]
    if labels(a) == labels(b):
        return "identical"
    if regs(a) == regs(b):
        return "identical up to register names"
    if sorted(regs(a)) == sorted(regs(b)):
        return f"the same {len(a)} instructions up to register names, in another order"
    return f"{len(a)} against {len(b)} instructions, not identical"


def part_resources(parent_root):
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        pres, pisa = compile_remarks(parent_root, t1)
        bres, bisa = compile_remarks(ROOT, t2)

    def row(n, v):
        return f"  {v['file']:<16}{n:<62} VGPRs {v['VGPRs']:>4}  SGPRs {v['SGPRs']:>4}  scratch {v['scratch']:>4}  LDS {v['LDS']:>6}  occupancy {v['occupancy']}"
    L = ["## 2. Code generation (cross-compiled, device code only; `unsigned short` is the raw bf16 storage type)",
         "Per file: hipcc with the flags of egoscaler_amd/build.py, --cuda-device-only -Rpass-analysis=kernel-resource-usage --save-temps", "Parent commit:"]
    same = [n for n, v in pres.items() if bres.get(n) == v and not re.search(r"rmsnorm|rope|adamw|qkv_finish", n)]     # the files' other kernels
    L += [row(n, v) for n, v in pres.items() if n not in same] + ["This tree:"] + [row(n, v) for n, v in bres.items() if n not in same]
    L.append(f"({len(same)} more instantiations in the three files, kernels this change does not touch: the same figures in both builds.)")
    worse, moved = [], []
    for n, v in pres.items():
        b = bres.get(replaced_by(n))
        if b is None:
            worse.append(f"{n}: no instantiation of this tree replaces it")
            continue
        if b["scratch"] > v["scratch"] or b["occupancy"] < v["occupancy"]:
            worse.append(f"{n} -> {replaced_by(n)}: scratch {v['scratch']} -> {b['scratch']}, occupancy {v['occupancy']} -> {b['occupancy']}")
        if (b["VGPRs"], b["SGPRs"], b["LDS"]) != (v["VGPRs"], v["SGPRs"], v["LDS"]):
            moved.append(f"  {n} -> {replaced_by(n)}: VGPRs {v['VGPRs']} -> {b['VGPRs']}, SGPRs {v['SGPRs']} -> {b['SGPRs']}, LDS {v['LDS']} -> {b['LDS']}")
    L.append(f"{len(pres)} instantiations at the parent, {len(bres)} in this tree; each of the parent's against the one that replaces it "
             "(rmsnorm_fwd_tail_kernel and slabs_rmsnorm_kernel -> rmsnorm_slabs_kernel; adamw*_ds_kernel<T, G> -> adamw*_kernel<T, G, float const*>):")
    L.append("Verdict: no instantiation has more scratch or a lower occupancy than the parent's." if not worse else "Verdict: WORSE than the parent:")
    L += ["  " + w for w in worse]
    L += ["Registers or LDS that moved (neither is a criterion):"] + (moved or ["  none"])
    L.append("ISA bodies, parent against this tree:")
    for n in sorted(pisa):
        if re.match(r"adamw(_vec4)?_kernel<", n) or n == "rmsnorm_fwd_kernel<unsigned short>":
            L.append(f"  {n:<62} {isa_equal(pisa[n], bisa[replaced_by(n)])}")
    return "\n".join(L) + "\n", not worse


# ---------------------------------------------------------------------------------------------------------------- bits
def child_bits(root, out_path):
    """One process, one build: every touched entry point on seeded inputs; writes [(label, sha256 of the output's bytes)] as JSON."""
    sys.path.insert(0, root)
    import torch
    from egoscaler_amd import ops
    assert torch.cuda.is_available(), "ab_row_kernels --parts bits needs a GPU"
    gen = torch.Generator().manual_seed(20240607)
    digests = []

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=gen).to(dtype).cuda()

    def put(label, *arrays):
        torch.cuda.synchronize()
        for i, a in enumerate(arrays):
            raw = a.detach().contiguous().cpu().view(torch.uint8).numpy()
            digests.append((f"{label} [{i}]", hashlib.sha256(raw).hexdigest()))

    def slab_tail(rows, row0, slices, cols):
        dev = rnd(slices, max(rows - row0, 1), cols)
        return dev, (row0, slices, dev.data_ptr())
    eps = 1e-6
    # RMSNorm: the small shapes of tests/test_gpu_row_pieces.py, then the workload's (cols 4096 at 5536 rows, a 96-row tail of 2 and 3 slices)
    norm_shapes = [(5, c, r0, sl) for c in (264, 2056, 4104) for r0 in (0, 2, 5) for sl in (1, 3)] + [(5536, 4096, 5440, 2), (5536, 4096, 5440, 3)]
    for dtype in (torch.bfloat16, torch.float32):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"
        for rows, cols, row0, sl in norm_shapes:
            lab = f"{tag} rows {rows} cols {cols} row0 {row0} slices {sl}"
            x, w, rstd = rnd(rows, cols, dtype=dtype), rnd(cols, dtype=dtype), torch.zeros(rows, device="cuda")
            if (row0, sl) in ((0, 1), (5440, 2)):
                put("egomi_rmsnorm_fwd " + lab, ops.rmsnorm(x, w, eps, rstd=rstd), rstd)
            for res in (None, rnd(rows, cols + 16, dtype=dtype)[:, :cols]):
                slabs, tail = slab_tail(rows, row0, sl, cols)
                xt, rs = x.clone(), torch.zeros(rows, device="cuda")
                y = ops.rmsnorm(xt, w, eps, rstd=rs, tail=tail, tail_residual=res)
                put(f"egomi_rmsnorm_fwd_tail {lab} residual {res is not None}", xt, y, rs)
            dy, rs, add = rnd(rows, cols, dtype=dtype), rnd(rows).abs() + 0.5, rnd(rows, cols, dtype=dtype)
            if (row0, sl) in ((0, 1), (5440, 2)):
                dw = rnd(cols)
                put("egomi_rmsnorm_bwd " + lab, ops.rmsnorm_bwd(dy, x, w, rs, dx_add=add, dw=dw), dw)
                seq, win = (7, 5) if rows == 5 else (692, 173)
                dw = rnd(cols)
                put(f"egomi_rmsnorm_bwd_rows {lab} seq {seq} win {win}", ops.rmsnorm_bwd(dy, x, w, rs, dx_add=add, dw=dw, window=(seq, win)), dw)
            slabs, tail = slab_tail(rows, row0, sl, cols)
            dyt, dw = dy.clone(), rnd(cols)
            put("egomi_rmsnorm_bwd_tail " + lab, ops.rmsnorm_bwd(dyt, x, w, rs, dx_add=add, dw=dw, tail=tail), dw, dyt)
        # the single-token step's norm: small with column views, and decode at B 256
        for rows, cols, sl, pad in [(5, c, s, 16) for c in (264, 2056, 4104) for s in (1, 3)] + [(256, 4096, 2, 0), (256, 4096, 3, 0)]:
            for res in (None, rnd(rows, cols + 16, dtype=dtype)[:, :cols]):
                slabs, w = rnd(sl, rows, cols), rnd(cols, dtype=dtype)
                xw, hw = rnd(rows, cols + pad, dtype=dtype), rnd(rows, cols + pad + 8, dtype=dtype)
                ops.slabs_rmsnorm(slabs, sl, res, w, eps, xw[:, pad // 2:pad // 2 + cols], hw[:, pad // 2:pad // 2 + cols])
                put(f"egomi_slabs_rmsnorm {tag} rows {rows} cols {cols} slices {sl} residual {res is not None}", xw, hw)
        # RoPE: vector and scalar form, both directions; the q|k|v tail form; small shapes and hd 128 with H 32 at the workload's rows
        for rows, S, off, H, hd in [(6, 3, 2, 2, 32), (6, 3, 2, 2, 128), (6, 3, 2, 2, 12), (5536, 692, 0, 32, 128)]:
            cos, sin = (t.cuda() for t in ops.rope_tables(S + off, hd, 10000.0))
            d = H * hd
            for inv in (False, True):
                buf = rnd(rows, 3 * d, dtype=dtype)
                ops.rope_(buf[:, d:2 * d], cos, sin, rows, S, off, H, hd, 3 * d, inverse=inv)
                put(f"egomi_rope {tag} rows {rows} H {H} hd {hd} inverse {inv}", buf)
            if hd == 12:
                continue
            for row0, sl in [(0, 1), (4, 3), (6, 1)] if rows == 6 else [(5440, 2), (5440, 3)]:
                slabs, tail = slab_tail(rows, row0, sl, 3 * d)
                buf = rnd(rows, 3 * d + 8, dtype=dtype)
                ops.rope_qkv_tail_(buf[:, :3 * d], cos, sin, rows, S, off, H, hd, 3 * d + 8, tail)
                put(f"egomi_rope_qkv_tail {tag} rows {rows} H {H} hd {hd} row0 {row0} slices {sl}", buf)
        # qkv_finish and its fp8 twin: small, and decode at B 256
        for B_, H, hd, pos, Smax, sls in [(3, 2, 32, 5, 8, (1, 3)), (3, 2, 128, 5, 8, (1, 3)), (256, 32, 128, 5, 8, (2, 3))]:
            cos, sin = (t.cuda() for t in ops.rope_tables(Smax, hd, 10000.0))
            d = H * hd
            for sl in sls:
                slabs = rnd(sl, B_, 3 * d)
                qkv, kc, vc = rnd(B_, 3 * d, dtype=dtype), rnd(B_, H, Smax, hd, dtype=dtype), rnd(B_, H, Smax, hd, dtype=dtype)
                ops.qkv_finish(slabs, sl, qkv, cos, sin, pos, kc, vc, B_, H, hd, Smax)
                put(f"egomi_qkv_finish {tag} B {B_} H {H} hd {hd} slices {sl}", qkv, kc, vc)
                qkv = rnd(B_, 3 * d, dtype=dtype)
                kc8, vc8 = (torch.zeros(B_, H, Smax, hd, dtype=torch.uint8, device="cuda") for _ in range(2))
                ks, vs = (torch.zeros(B_, H, Smax, device="cuda") for _ in range(2))
                ops.qkv_finish_fp8(slabs, sl, qkv, cos, sin, pos, kc8, vc8, ks, vs, B_, H, hd, Smax)
                put(f"egomi_qkv_finish_fp8 {tag} B {B_} H {H} hd {hd} slices {sl}", qkv, kc8, vc8, ks, vs)
    # AdamW: the four entries (host / device scale x fp32 / bf16 gradient), aligned and at an odd element offset, with and without the bf16 copy
    for n in (1003, 4096 * 11008):
        vals = [torch.randn(n, generator=gen) for _ in range(4)]
        scale = torch.full((1,), 0.5, device="cuda")
        for gdt in (torch.float32, torch.bfloat16):
            for off in (0, 1):
                for with_copy in (False, True):
                    for dev_scale in (False, True):
                        def at(v, dtype=torch.float32):
                            buf = torch.zeros(n + 8, dtype=dtype, device="cuda")
                            buf[off:off + n] = v.to(dtype)
                            return buf[off:off + n]
                        master, m, v, g = at(vals[0]), at(vals[1]), at(vals[2].abs()), at(vals[3], gdt)
                        cp = at(torch.zeros(n), torch.bfloat16) if with_copy else None
                        for step in (1, 2):
                            ops.adamw(master, cp, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.5, grad_scale_dev=scale if dev_scale else None)
                        put(f"egomi_adamw{'_g16' if gdt == torch.bfloat16 else ''}{'_ds' if dev_scale else ''} n {n} offset {off} copy {with_copy}",
                            master, m, v, *([cp] if with_copy else []))
                        del master, m, v, g, cp
    with open(out_path, "w") as f:
        json.dump(digests, f)
    print(f"BITS {len(digests)} arrays", flush=True)


def part_bits(parent_root):
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, root in (("parent", parent_root), ("branch", ROOT)):
            out = os.path.join(tmp, name + ".json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bits", root, out], capture_output=True, text=True, cwd=root, timeout=900)
            if r.returncode != 0:                                      # (a child that hangs or faults ends the tool)
                raise SystemExit(f"bits child of the {name} build failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            got[name] = [tuple(x) for x in json.load(open(out))]
    p, b = got["parent"], got["branch"]
    diff = [f"  {lp}: parent {hp[:16]} branch {hb[:16]}" for (lp, hp), (lb, hb) in zip(p, b) if (lp, hp) != (lb, hb)]
    per = {}
    for lab, _ in b:
        per[lab.split()[0]] = per.get(lab.split()[0], 0) + 1
    ok = len(p) == len(b) and not diff
    L = ["## 1. Bits: the parent's library against this tree's, one MI355X",
         "One fresh child process per build (its own tree on sys.path), the same inputs from torch's CPU generator (seed 20240607), every touched entry",
         "point in bf16 and fp32 at the small shapes of tests/test_gpu_row_pieces.py and at the workload's (cols 4096 at 5536 rows with a 96-row tail of 2 and",
         "3 slices; hd 128 with H 32; decode at B 256; AdamW at n = 4096 * 11008, aligned and at an odd offset, with and without the bf16 copy, two steps);",
         "SHA-256 of the raw bytes of every output array.  Arrays per entry point:"]
    L += [f"  {k:<28}{v:>5}" for k, v in per.items()]
    L.append(f"Verdict: {len(b)} arrays compared ({len(p)} from the parent); " + ("ALL BYTE-EQUAL." if ok else f"{len(diff)} DIFFER:"))
    return "\n".join(L + diff) + "\n", ok


# ---------------------------------------------------------------------------------------------------------------- time
def child_adamw(root):
    """egomi_adamw / _g16 over the gradient table of the frozen and the LoRA set-up at 7B (tools/bench_grad_clip.py run_tables)."""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import bench_grad_clip
    rows = bench_grad_clip.run_tables(["frozen", "lora"], 7)
    print("RESULT " + json.dumps({r["table"]: r["adamw_us"][0] for r in rows}), flush=True)


def part_time(parent_root, arms, rounds, step_modes):
    def one(cmd, root, pick):
        r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, cwd=root, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("{", "RESULT "))]
        if r.returncode != 0 or not lines:                             # (a child that hangs or faults ends the tool)
            raise SystemExit(f"{' '.join(cmd)} in {root} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return pick(json.loads(lines[-1].removeprefix("RESULT ")))
    me = os.path.abspath(__file__)
    plan = []                                                          # (figure, command, {key: pick})
    if "bench" in arms:
        plan.append(("bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-extras: ms/step",
                     ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-extras"], lambda d: d["ms_per_step"]))
    if "decode" in arms:
        plan.append(("tools/bench_decode.py: ms/step (bs 256, 32 greedy steps in one graph)", ["tools/bench_decode.py"], lambda d: d["ms_per_step"]))
    if "adamw" in arms:
        for t in ("frozen", "lora"):
            plan.append((f"bench_grad_clip AdamW, {t} table: us per pass", [me, "--child-adamw"], lambda d, t=t: d[t]))
    if "step" in arms:
        for mode in step_modes:
            plan.append((f"bench_grad_clip step, {mode}: ms/step", ["tools/bench_grad_clip.py", "--child", "ROOT", mode, "off", "10", "3"],
                         lambda d: d["ms_per_step"]))
    L = [f"## 3. Speed: both builds alternated, {rounds} rounds each, one MI355X, one fresh process per figure and round (order per round: parent, branch)",
         "p.spread = the parent's max - min over its rounds; verdict `inside`: branch median - parent median <= p.spread.",
         f"{'figure':<76}{'parent rounds':<32}{'branch rounds':<32}{'p.median':>10}{'b.median':>10}{'p.spread':>10}  verdict"]
    ok, cache = True, {}
    for fig, cmd, pick in plan:
        runs = {"parent": [], "branch": []}
        for rd in range(rounds):
            for name, root in (("parent", parent_root), ("branch", ROOT)):
                key = (tuple(cmd), name, rd)
                if cmd[-1] == "--child-adamw" and key in cache:        # one process measures both tables
                    runs[name].append(pick(cache[key]))
                    continue
                full = [root if c == "ROOT" else c for c in cmd] + ([root] if cmd[-1] == "--child-adamw" else [])
                cache[key] = one(full, root, lambda d: d)
                runs[name].append(pick(cache[key]))
                print(f"[{fig}] {name}: {runs[name][-1]}", file=sys.stderr, flush=True)
        pm, bm = statistics.median(runs["parent"]), statistics.median(runs["branch"])
        spread = max(runs["parent"]) - min(runs["parent"])
        inside = bm - pm <= spread
        ok &= inside
        L.append(f"{fig:<76}{', '.join(f'{x:g}' for x in runs['parent']):<32}{', '.join(f'{x:g}' for x in runs['branch']):<32}{pm:>10g}{bm:>10g}{spread:>10.3g}  "
                 + ("inside" if inside else f"SLOWER by {100 * (bm - pm) / pm:.2f} %"))
    return "\n".join(L) + "\n", ok


# ---------------------------------------------------------------------------------------------------------------- the report
def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child-bits":
        return child_bits(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 2 and sys.argv[1] == "--child-adamw":
        return child_adamw(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True, help="a built checkout of the parent commit")
    ap.add_argument("--parts", default="resources,bits,time")
    ap.add_argument("--arms", default="bench,decode,adamw,step", help="the figures of the time part")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-modes", default="frozen,unfrozen")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_pieces_ab.txt"))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_root)
    parts = a.parts.split(",")
    sections, ok = {}, True
    if os.path.exists(a.out):                                          # keep the sections of parts not run now
        for sec in re.split(r"(?m)^(?=## \d\. )", open(a.out).read())[1:]:
            sections[sec[3]] = sec.rstrip("\n") + "\n"
    for num, name, fn in (("1", "bits", lambda: part_bits(parent)), ("2", "resources", lambda: part_resources(parent)),
                          ("3", "time", lambda: part_time(parent, a.arms.split(","), a.rounds, a.step_modes.split(",")))):
        if name in parts:
            sections[num], good = fn()
            ok &= good
    text = ("# The row kernels on csrc/row_pieces.h (slab sum, round-as-stored, RMSNorm row, RoPE pair; one RMSNorm-from-slabs kernel; one AdamW kernel\n"
            "# family) against the parent commit: output bits, code generation, speed.  tools/ab_row_kernels.py --parent-root <parent checkout>\n\n"
            + "\n".join(sections[k] for k in sorted(sections)))
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
