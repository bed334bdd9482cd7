#!/usr/bin/env python3
"""Static instruction budget of the Connect4 rollout loop (CPU only: a cross-compile).

    python tools/isa_budget.py [--asm FILE] [--label TEXT] [--kernel KEY] [--instances]

Compiles zeroclone_amd/csrc/c4_search.hip to gfx950 assembly with build.py's flags (ZC_CFLAGS
honoured; --asm FILE reads an assembly file made that way instead), finds the rollout loops of
c4_selfplay_kernel<false, kModeCarry, true> (the headline's instance: exact rollouts, pooled
carry, planned flush; --kernel KEY: the instance whose mangled name holds KEY) by the win test's ds_permute_b32 + v_permlane32_swap — one test in
a loop over blocks inside the loop over leaves, or two when a rollout's first block stands in
the leaf loop itself and the others in a loop of their own — and prints

  * per basic block of the leaf loop: SALU / VALU / LDS / other instruction counts (other =
    waits, nops, branches, priorities, vector memory), its loop depth and successors;
  * the sums along three paths, each the cheapest that fits its description:
      win       leaf prologue -> one block without a fill -> exit to the next leaf
                (the exit is the cheapest way from the win test to the next leaf that does
                not start another block: the win exit, which the board-full exit shares or ties)
      absorbed  the same with one absorbed fill (the block passes two prefix sums)
      continue  one block without a fill that goes on to another: from one win test round the
                block loop to the next (told from the exit by its LDS read of the next legal
                set's order words)
    (no window advance / stream refill and no empty view on any of them);
  * the stream: the instructions of the leaf head's refill (the code the "enough words ahead?"
    test branches around: the 64-word window advance of the register-window stream, the
    224-word bulk step of the draw-ring stream), all of its branches counted, per step and
    per 64 generated words, and the instructions of a view (from the refill's join to the
    lane's word: a ds_bpermute_b32 of the window registers, or a byte read of the draw ring);
  * the flush outside the rollouts (flush_budget below): a level of the prefetching walk, stage
    1a of the planned flush, the draw table + chase, stages 2-3, backup + publish (every block
    once, and the executed path's bounds: the longest way through the planned backup, every
    lane-parallel section and mode test entered, and the shortest, all of them skipped), the serial loop's trip for a dead leaf, and per region the spilled-scalar
    reloads (v_readlane_b32 sN, vK, imm from a VGPR that only v_writelane_b32 with an
    immediate lane ever writes: the allocator's SGPR spill registers);
  * next_free_vgpr and the private segment size of that instance and of the planned lockstep
    search, c4_search_kernel<false, false, true>;
  * --instances: registers, spills and scratch of every search instance, and whether each
    holds the other flush path's code (select_flush's ds_add backup in a planned instance).

profiles/c4_rollout_isa_budget.txt and profiles/c4_flush_isa_budget.txt keep the output for the
code before and after a change.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL = "c4_selfplay_kernelILb0ELi3ELb1EE"   # <PHILOX false, kModeCarry, PLANNED true>
ALSO = ["c4_search_kernelILb0ELb0ELb1EE"]     # <STAMP false, PHILOX false, PLANNED true>
OLD_NAMES = {KERNEL: "c4_selfplay_kernelILb0EE", ALSO[0]: "c4_search_kernelILb0ELb0EE"}  # before the mode split
OTHER = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_setprio", "s_sleep", "s_endpgm", "s_barrier",
         "s_setpc", "s_sendmsg", "s_trap", "s_inst_prefetch", "s_code_end")


def compile_asm(path):
    from zeroclone_amd import build as zb
    src = "c4_search.hip"
    cmd = [zb.hipcc(), f"--offload-arch={zb.ARCH}", *zb.FLAGS, *zb.SOURCE_FLAGS.get(src, []),
           *os.environ.get("ZC_CFLAGS", "").split(), "--cuda-device-only", "-S",
           os.path.join(zb.CSRC, src), "-o", path]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def kind(op):
    if op.startswith(OTHER):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    return "other"


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ, self.falls = name, [], [], True
        self.header_of = None   # depth, when this block heads a loop
        self.loop = None        # innermost loop header this block is in (its own name for a header)
        self.parents = {}       # header blocks only: depth -> enclosing header

    def counts(self):
        c = dict(salu=0, valu=0, lds=0, other=0)
        for op, _ in self.ins:
            c[kind(op)] += 1
        return c

    def n(self):
        return len(self.ins)


def parse_function(lines, key):
    """Basic blocks of the function whose symbol contains `key`, in layout order."""
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l))
    fn = re.match(r"^(\S+):", lines[start]).group(1)
    blocks, cur, fnum = [], Block("entry"), None
    blocks.append(cur)
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\.L(BB(\d+)_\d+):(.*)", l) or re.match(r"^; %bb\.(\d+):(.*)", l)
        if m:
            if m.re.pattern.startswith(r"^\.L"):
                name, fnum, rest = m.group(1), m.group(2), m.group(3)
            else:
                name, rest = f"BB{fnum if fnum is not None else '?'}_{m.group(1)}", m.group(2)
            cur = Block(name)
            blocks.append(cur)
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", rest)
            if h:
                cur.loop = h.group(1)
            l = rest  # a loop header's comment starts on the label's line
        s = l.strip()
        if s.startswith(";"):
            h = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", s)
            if h:
                cur.parents[int(h.group(2))] = h.group(1)
            h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
            if h:
                cur.header_of = int(h.group(1))
                cur.loop = cur.name
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        cur.ins.append((op, s))
        if op.startswith(("s_cbranch", "s_branch")):
            t = s.split()[1]
            cur.succ.append(t[2:] if t.startswith(".L") else t)
        if op in ("s_branch", "s_endpgm"):
            cur.falls = False
    # "%bb.N" blocks seen before the first label get the function number now
    for b in blocks:
        if b.name.startswith("BB?_"):
            b.name = f"BB{fnum}_" + b.name[4:]
    for i, b in enumerate(blocks):
        if b.falls and i + 1 < len(blocks):
            b.succ.append(blocks[i + 1].name)
    return fn, blocks


def loop_chain(byname, b):
    """Headers of the loops around block b, innermost first."""
    out, h = [], b.loop
    while h:
        out.append(h)
        hb = byname[h]
        h = hb.parents.get(hb.header_of - 1)
    return out


def all_paths(byname, src, dst, allowed):
    """Simple paths src .. dst (both included; a cycle when they are the same) through `allowed`."""
    out, stack = [], [(src, [src])]
    while stack:
        node, path = stack.pop()
        for s in byname[node].succ:
            if s == dst:
                out.append(path + [s])
            elif s in allowed and s not in path:
                stack.append((s, path + [s]))
    return out


def cost(byname, path):
    return sum(byname[b].n() for b in path)


def fmt_counts(byname, path):
    c = dict(salu=0, valu=0, lds=0, other=0)
    for b in path:
        for k, v in byname[b].counts().items():
            c[k] += v
    return f"SALU {c['salu']:3d}  VALU {c['valu']:3d}  LDS {c['lds']:2d}  other {c['other']:2d}  total {sum(c.values()):3d}"


def has(byname, path, text):
    return sum(text in s for b in path for _, s in byname[b].ins)


# what marks the stream's refill code, and the words one pass of it generates: the tempering
# mask of the register-window stream (one 64-word window per advance), the draw extraction's
# mask of the draw-ring stream (kLStep = 224 words per step)
STREAM_MARKS = {"0x9d2c5680": 64, "0x80004000": 224}
VIEW_OPS = ("ds_bpermute_b32", "ds_read_u8")


def stream_budget(blocks, byname, head, out):
    """The refill the leaf head branches around, and the view after it (see the module docstring)."""
    order = [b.name for b in blocks]
    vi = next(i for i, n in enumerate(head) if any(op in VIEW_OPS for op, _ in byname[n].ins))
    view, test = byname[head[vi]], byname[head[vi - 1]]
    lo, hi = order.index(test.name) + 1, order.index(view.name)
    region = order[lo:hi]   # the test falls into the refill and branches to the view
    if view.name not in test.succ or not region:
        raise SystemExit("isa_budget: no refill between the stream test and the view")
    words = next((w for b in region for m, w in STREAM_MARKS.items() if has(byname, [b], m)), None)
    if words is None:
        raise SystemExit("isa_budget: the refill region holds no stream constant")
    n = cost(byname, region)
    nview = 1 + next(i for i, (op, _) in enumerate(view.ins) if op in VIEW_OPS)
    print(f"stream refill  {fmt_counts(byname, region)}  per {words} words, {n * 64 / words:.1f} per 64 words"
          f"  ({test.name} -> {' '.join(region)})", file=out)
    print(f"stream view    {nview:3d} instructions  ({' '.join(s.split()[0] for _, s in view.ins[:nview])})", file=out)
    return {"refill": n, "words": words, "per64": n * 64 / words, "view": nview}


def operands(op, s):
    return [t.strip() for t in s[len(op):].split(",")]


def vregs(tok):
    """The VGPR numbers of an operand: v5 -> [5], v[4:7] -> [4, 5, 6, 7], anything else -> []."""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return [int(m.group(1))]
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    return list(range(int(m.group(1)), int(m.group(2)) + 1)) if m else []


def spill_vgprs(blocks):
    """The allocator's SGPR spill registers: VGPRs written by v_writelane_b32 with an immediate lane
    and by nothing else (the code's own lane writes select the lane from an SGPR or M0)."""
    lanes, other = set(), set()
    for b in blocks:
        for op, s in b.ins:
            ops = operands(op, s)
            if op == "v_writelane_b32" and len(ops) == 3 and re.fullmatch(r"\d+", ops[2]):
                lanes.update(vregs(ops[0]))
            elif op.startswith(("v_swap", "v_permlane32_swap", "v_permlane16_swap")):
                other.update(v for t in ops for v in vregs(t))
            elif op.startswith(("v_", "ds_", "global_load", "buffer_load", "scratch_load", "flat_load")):
                other.update(vregs(ops[0]))
    return lanes - other


def reloads(byname, names, spill):
    """Spilled scalars read back in these blocks."""
    n = 0
    for b in names:
        for op, s in byname[b].ins:
            ops = operands(op, s)
            if (op == "v_readlane_b32" and len(ops) == 3 and re.fullmatch(r"\d+", ops[2])
                    and set(vregs(ops[1])) & spill):
                n += 1
    return n


def longest_path(byname, pos, names, src, dst, longest=True):
    """The costliest (or cheapest) way src .. dst through `names` along forward (layout-order) edges;
    None: no way."""
    memo = {}

    def go(n):
        if n not in memo:
            best = None
            for s in byname[n].succ:
                if s == dst:
                    cand = []
                elif s in names and pos[s] > pos[n]:
                    cand = go(s)
                else:
                    continue
                if cand is not None and (best is None or (cost(byname, cand) > cost(byname, best)) == longest):
                    best = cand
            memo[n] = None if best is None else [n] + best
        return memo[n]

    return go(src)


def flush_budget(blocks, byname, Lh, out):
    """The flush outside the rollouts (select_flush_plan, backup, publish), by the same columns.

    The flush loop is the loop around the leaf loop.  In it, in layout order: the prefetching
    walk (the loop whose latch moves the chosen child's slots over with three ds_bpermute_b32;
    a level = the cheapest trip round it through the UCT scores, told by their square root:
    v_sqrt_f32 for the fp32 decision, v_rsq_f64 for fp64), stage 1a (the flush loop's own blocks
    between the walk and the chase, each once: X0's step, the terminal node's and, when the
    chain is built by runs, one run with its fill; and where the compiler kept a loop there, the
    per-node chain, the cheapest trip round it = one more chain node), the draw table + chase
    (the block of unrolled s_bitset1_b64), stages 2-3
    (the flush loop's own blocks from there to the rollouts, each once, rare paths included) and
    backup + publish (every block after the leaf loop, each once)."""
    pos = {b.name: i for i, b in enumerate(blocks)}
    nops = lambda b, op: sum(o == op for o, _ in b.ins)
    chase = next(b for b in blocks if nops(b, "s_bitset1_b64") >= 16)
    # the innermost loop around both the leaf loop and the chase
    F = next(h for h in loop_chain(byname, byname[Lh]) if h in loop_chain(byname, chase))
    inF = [b for b in blocks if F in loop_chain(byname, b)]
    inside = lambda h: [b for b in inF if h in loop_chain(byname, b)]
    latch = next(b for b in inF if nops(b, "ds_bpermute_b32") >= 3 and b.loop != F and pos[b.name] < pos[chase.name])
    W = latch.loop
    wnames = {b.name for b in inside(W)}
    trips = all_paths(byname, W, W, wnames)
    res = {}

    def trip_through(mark):
        ps = [p[:-1] for p in trips if has(byname, p[:-1], mark)]
        return min(ps, key=lambda p: cost(byname, p)) if ps else None

    fast, slow = trip_through("v_sqrt_f32"), trip_through("v_rsq_f64")
    print(f"flush loop {F}, walk loop {W}, chase in {chase.name}", file=out)
    for name, p in (("walk level, fp32 decision", fast), ("walk level, fp64 scores", slow)):
        if p:
            fp64 = sum(op.endswith("_f64") or "_f64_" in op for b in p for op, _ in byname[b].ins)
            print(f"flush {name:<28} {fmt_counts(byname, p)}  (fp64 {fp64})  " + " ".join(p), file=out)
            res[name] = cost(byname, p)
    wend = max(pos[n] for n in wnames)
    once = [b.name for b in inF if b.loop == F and wend < pos[b.name] < pos[chase.name]]
    print(f"flush {'stage 1a, blocks once':<28} {fmt_counts(byname, once)}  {len(once)} blocks", file=out)
    res["stage1a"] = cost(byname, once)
    between = {b.loop for b in inF if b.loop not in (F, W) and wend < pos[b.name] < pos[chase.name]}
    if between:
        S = max(between, key=lambda h: sum(b.n() for b in inside(h)))
        snames = {b.name for b in inside(S)}
        steps = [p[:-1] for p in all_paths(byname, S, S, snames)]
        p = min(steps, key=lambda p: cost(byname, p))
        print(f"flush {'stage 1a, one step':<28} {fmt_counts(byname, p)}  " + " ".join(p), file=out)
        res["step"] = cost(byname, p)
    print(f"flush {'draw table + chase':<28} {fmt_counts(byname, [chase.name])}  {chase.name}", file=out)
    first_leaf = min(pos[b.name] for b in inF if Lh in loop_chain(byname, b))
    last_leaf = max(pos[b.name] for b in inF if Lh in loop_chain(byname, b))
    st23 = [b.name for b in inF if b.loop == F and pos[chase.name] < pos[b.name] < first_leaf]
    tail = [b.name for b in inF if pos[b.name] > last_leaf]
    print(f"flush {'stages 2-3':<28} {fmt_counts(byname, st23)}  {len(st23)} blocks", file=out)
    print(f"flush {'backup + publish':<28} {fmt_counts(byname, tail)}  {len(tail)} blocks", file=out)
    res.update(chase=chase.n(), stages23=cost(byname, st23), tail=cost(byname, tail))
    # the executed path of backup + publish lies between the longest way from the leaf loop's exit
    # round to the flush loop's header (every lane-parallel section entered, X0 rewritten, every
    # mode's test taken) and the shortest (all of them skipped)
    # (it starts at the first of the flush loop's own blocks there: rare blocks of the leaf loop
    # can be laid out after its last common one; the loops of the flush that is not planned are
    # left out, so in a kernel that holds both flushes this is the planned one's path)
    own = [n for n in tail if byname[n].loop == F]
    if own:
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(blocks)))
        # through the planned backup's prefix sum (row_bcast:31 ends scan_add32) when there is one
        scan = next((n for n in own if has(byname, [n], "row_bcast:31")), None)
        for longest, name, key in ((True, "backup + publish, longest", "tail_run"),
                                   (False, "backup + publish, shortest", "tail_min")):
            if scan and scan != own[0]:
                head = longest_path(byname, pos, set(own), own[0], scan, longest)
                rest = longest_path(byname, pos, set(own), scan, F, longest)
                run = head + rest if head and rest else None
            else:
                run = longest_path(byname, pos, set(own), own[0], F, longest)
            if run:
                print(f"flush {name:<28} {fmt_counts(byname, run)}  {len(run)} blocks", file=out)
                res[key] = cost(byname, run)
    # a dead leaf (won or full at its start): the serial loop's trip that passes no win test
    in_leaf = {b.name for b in inF if Lh in loop_chain(byname, b)}
    tests = {b.name for b in inF if any(op == "ds_permute_b32" for op, _ in b.ins)
             and any(op.startswith("v_permlane32_swap") for op, _ in b.ins)}
    calm = {n for n in in_leaf - tests if not any(has(byname, [n], m) for m in STREAM_MARKS)}
    dead = [p[:-1] for p in all_paths(byname, Lh, Lh, calm)]
    if dead:
        p = min(dead, key=lambda p: cost(byname, p))
        print(f"flush {'dead leaf, serial loop trip':<28} {fmt_counts(byname, p)}  " + " ".join(p), file=out)
        res["dead_leaf"] = cost(byname, p)
    else:
        print(f"flush {'dead leaf, serial loop trip':<28} none: every trip of the leaf loop passes a win test", file=out)
        res["dead_leaf"] = 0
    # spilled scalars read back, per region
    spill = spill_vgprs(blocks)
    regions = (("walk level loop", sorted(wnames)), ("leaf + block loops", sorted(in_leaf)),
               ("stages 1a-3", once + [chase.name] + st23), ("backup + publish", tail),
               ("whole flush loop", [b.name for b in inF]))
    print(f"spill registers: {' '.join('v%d' % v for v in sorted(spill)) or 'none'}", file=out)
    res["reloads"] = {}
    for name, names in regions:
        res["reloads"][name] = reloads(byname, names, spill)
        print(f"spilled-scalar reloads, {name:<20} {res['reloads'][name]:3d}", file=out)
    return res


def instances(lines, out):
    """Every search instance: registers, SGPR spills, scratch, and the flush paths its body holds
    (planned: select_flush_plan's unrolled chase; not planned: the atomic backup's ds_add)."""
    text = "\n".join(lines)
    meta = text[text.index("amdhsa.kernels"):]
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*(c4_(?:search|selfplay|walk)_kernelI\w+?E)EvNS\S*)\n(.*?)\.end_amdhsa_kernel",
                         text, re.S):
        sym, key, body = m.group(1), m.group(2), m.group(3)
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        ps = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        md = re.search(r"\.name:\s+" + re.escape(sym) + r"\n.*?\.sgpr_spill_count:\s+(\d+)", meta, re.S)
        ops = [op for b in parse_function(lines, key + "EvNS")[1] for op, _ in b.ins]
        res[key] = dict(vgprs=vg, scratch=ps, sgpr_spills=int(md.group(1)) if md else -1, n=len(ops),
                        chase=ops.count("s_bitset1_b64"), ds_add=sum(op.startswith("ds_add") for op in ops))
        r = res[key]
        print(f"{key:<36} vgprs {vg:3d}  scratch {ps:3d}  sgpr spills {r['sgpr_spills']:3d}  instructions {r['n']:5d}"
              f"  chase s_bitset1 {r['chase']:2d}  backup ds_add {r['ds_add']:2d}", file=out)
    return res


def analyse(lines, out, kernel=None):
    kernel = asked = kernel or KERNEL
    if not any(re.match(r"^_Z\S*" + re.escape(kernel), l) for l in lines):  # an assembly from before the mode split
        kernel = OLD_NAMES.get(kernel, kernel)
    fn, blocks = parse_function(lines, kernel)
    byname = {b.name: b for b in blocks}
    depth = lambda b: byname[b.loop].header_of if b.loop else 0
    tests = [b for b in blocks if any(op == "ds_permute_b32" for op, _ in b.ins)
             and any(op.startswith("v_permlane32_swap") for op, _ in b.ins)]
    # one win test: a loop over blocks inside the loop over leaves.  Two: a rollout's first
    # block stands in the leaf loop itself, the others in a loop of their own.
    P1 = min(tests, key=depth)
    P2 = max(tests, key=depth)
    if len(tests) == 1:
        B, Lh = loop_chain(byname, P1)[:2]
    else:
        B, Lh = loop_chain(byname, P2)[0], loop_chain(byname, P1)[0]
    in_leaf = [b for b in blocks if Lh in loop_chain(byname, b)]
    print(f"kernel {fn}", file=out)
    print(f"leaf loop {Lh}, block loop {B}, win test in " + " ".join(t.name for t in tests), file=out)
    print(f"{'block':<12}{'depth':>5}{'SALU':>6}{'VALU':>6}{'LDS':>5}{'other':>6}{'total':>6}  successors", file=out)
    for b in in_leaf:
        c = b.counts()
        print(f"{b.name:<12}{depth(b):>5}{c['salu']:>6}{c['valu']:>6}{c['lds']:>5}{c['other']:>6}{b.n():>6}  "
              + " ".join(b.succ), file=out)

    def best(paths, what):
        if not paths:
            raise SystemExit(f"isa_budget: no path for {what}")
        return min(paths, key=lambda p: cost(byname, p))

    # no path advances the window / refills the stream or meets an empty view (the temper's
    # constant, or the draw extraction's, marks both)
    calm = {b.name for b in in_leaf if not any(has(byname, [b.name], m) for m in STREAM_MARKS)}
    testnames = {t.name for t in tests}
    # leaf header .. win test: the leaf's prologue and one block, by the prefix sums it passes
    head = all_paths(byname, Lh, P1.name, calm - testnames)
    nofill = best([p for p in head if has(byname, p, "row_bcast:31") == 1], "block without fill")
    fill = best([p for p in head if has(byname, p, "row_bcast:31") == 2], "block with an absorbed fill")
    # after the win test, to the next leaf: going on reads the next legal set's order words
    # from LDS (and passes another win test), the exit reads nothing
    quiet = {n for n in calm - testnames if not has(byname, [n], "ds_read")}
    ex = best([p[1:-1] for p in all_paths(byname, P1.name, Lh, quiet)], "exit")
    # a block that goes on: the cycle from one win test of the block loop to the next
    in_loop = {n for n in calm if B in loop_chain(byname, byname[n])}
    cyc = best([p[1:] for p in all_paths(byname, P2.name, P2.name, in_loop)
                if has(byname, p[1:], "ds_read") and has(byname, p[1:], "row_bcast:31") == 1], "continue")
    paths = [("win", nofill + ex), ("absorbed", fill + ex), ("continue", cyc)]
    print(file=out)
    for name, parts in (("leaf + block, no fill", nofill), ("leaf + block, absorbed fill", fill),
                        ("exit to the next leaf", ex), ("block that goes on", cyc)):
        print(f"part {name:<28}{cost(byname, parts):>4}  " + " ".join(parts), file=out)
    print(file=out)
    for name, p in paths:
        print(f"path {name:<9} {fmt_counts(byname, p)}", file=out)
    print(file=out)
    res = {name: cost(byname, p) for name, p in paths}
    res["stream"] = stream_budget(blocks, byname, nofill, out)
    print(file=out)
    try:
        res["flush"] = flush_budget(blocks, byname, Lh, out)
    except (StopIteration, ValueError, IndexError) as e:  # its markers moved: the rollout budget still stands
        print(f"flush section: markers not found ({type(e).__name__})", file=out)
    print(file=out)
    text = "\n".join(lines)
    for key in [asked] + ALSO:
        m = (re.search(r"\.amdhsa_kernel (\S*" + re.escape(key) + r"\S*)\n(.*?)\.end_amdhsa_kernel", text, re.S) or
             re.search(r"\.amdhsa_kernel (\S*" + re.escape(OLD_NAMES.get(key, key)) + r"\S*)\n(.*?)\.end_amdhsa_kernel", text, re.S))
        body = m.group(2)
        vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)
        ps = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)
        print(f"{key}: next_free_vgpr {vg}  private_segment_fixed_size {ps}", file=out)
        res[key] = (int(vg), int(ps))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="analyse this assembly file instead of compiling")
    ap.add_argument("--label", help="a heading printed first (e.g. the commit)")
    ap.add_argument("--kernel", help="part of the mangled name of the self-play instance to analyse")
    ap.add_argument("--instances", action="store_true", help="also list every search instance")
    a = ap.parse_args()
    if a.asm:
        lines = open(a.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "c4_search.s")
            compile_asm(path)
            lines = open(path).read().splitlines()
    if a.label:
        print(f"== {a.label}")
    analyse(lines, sys.stdout, a.kernel)
    if a.instances:
        print()
        instances(lines, sys.stdout)


if __name__ == "__main__":
    main()
