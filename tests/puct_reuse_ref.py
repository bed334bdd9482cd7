"""Tree reuse of the Connect4 PUCT search (zc_c4_puct_begin_reuse, c4_puct.hip) in executable
form, on oracle.puct_ref's Node and C4Rules (TEST INFRASTRUCTURE ONLY): the search loop of
puct_ref.search restated so that it takes and returns a root Node, the rule that picks the
new root, and the re-root of a zc_debug_c4_puct_tree dump as a pure function."""
import math

from oracle.puct_ref import C4Rules, Capacity, Node


def count_slots(node):
    return len(node.moves) + sum(count_slots(ch) for ch in node.child if ch is not None)


def search(root, sims, bs, c, value_fn, prior_fn, rules=C4Rules, reused=False, max_level=None, slot_cap=None,
           created=None, mutation=None):
    """puct_ref.search from `root` (a fresh Node, or a kept one with reused=True: flush 0, the
    root's own evaluation, then has no leaf, so the search adds sims - 1 visits below it).
    Returns (root moves, root visits, chosen index); the tree stays in `root`.

    max_level / slot_cap: puct_ref.search's two limits (a kept tree's slots count as taken);
    they raise puct_ref.Capacity.  created: a list that takes the nodes this search creates, in
    creation order.  mutation: a deliberately wrong search for the mutation checks — "sign" (the
    backup does not alternate the value's sign), "loss" (the virtual loss is not undone) or
    "once" (a leaf pending more than once in a flush is backed up once)."""
    slots = count_slots(root)
    flushes = 1 + (sims - 1 + bs - 1) // bs
    for f in range(flushes):
        if f == 0:
            nb = 0 if reused else 1
        else:
            nb = max(0, min(bs, sims - 1 - (f - 1) * bs))
        leaves, made = [], []
        for _ in range(nb):
            if f == 0:
                leaves.append((root, []))
                continue
            node, path = root, []
            while len(node.moves) and node.evaluated:
                if max_level is not None and len(path) >= max_level:
                    raise Capacity(f, "depth")
                sq = math.sqrt(float(sum(node.N)))
                best, bv = -1, -math.inf
                for j in range(len(node.moves)):
                    q = node.W[j] / node.N[j] if node.N[j] > 0 else 0.0
                    v = q + c * node.P[j] * sq / float(1 + node.N[j])
                    if v > bv:
                        bv, best = v, j
                node.N[best] += 1
                node.W[best] -= 1.0
                path.append((node, best))
                if node.child[best] is None:
                    node.child[best] = Node(rules.play(node.s, node.moves[best]), rules)
                    node = node.child[best]
                    made.append(node)
                    break
                node = node.child[best]
            leaves.append((node, path))
        if created is not None:
            created.extend(made)
        for node in made:
            slots += len(node.moves)
            if slot_cap is not None and slots > slot_cap:
                raise Capacity(f, "slots")
        seen = set()
        for node, path in leaves:
            if mutation == "once":
                if id(node) in seen:
                    continue
                seen.add(id(node))
            if len(node.moves) == 0:
                v = -1.0 if rules.win(node.s) else 0.0
            else:
                v = value_fn(node.s)
                if not node.evaluated:
                    node.P = prior_fn(node)
                    node.evaluated = True
            d = len(path)
            for l, (par, a) in enumerate(path, start=1):
                r = v if (d - l) % 2 == 0 or mutation == "sign" else -v
                par.W[a] = par.W[a] + (0.0 if mutation == "loss" else 1.0) - r
    best, bn = -1, -1
    for j, n in enumerate(root.N):
        if n > bn:
            bn, best = n, j
    return root.moves, root.N, best


def advance(root, state):
    """The node of `root`'s tree holding `state`: the first child in slot order that does,
    else the first grandchild (child slot, then grandchild slot); None when there is none, when
    it was never evaluated or has no moves.  The root itself never matches."""
    found = None
    for ch in root.child:
        if ch is not None and ch.s == state:
            found = ch
            break
    if found is None:
        for ch in root.child:
            if ch is None:
                continue
            for gc in ch.child:
                if gc is not None and gc.s == state:
                    found = gc
                    break
            if found is not None:
                break
    if found is None or not found.evaluated or len(found.moves) == 0:
        return None
    return found


def count_nodes(node):
    return 1 + sum(count_nodes(ch) for ch in node.child if ch is not None)


def next_root(root, state, sims, max_nodes, rules=C4Rules):
    """(root of the next search of `state`, nodes kept): the kept subtree when advance() finds
    one and kept + sims - 1 <= max_nodes, else a fresh Node and 0."""
    if root is not None:
        nr = advance(root, state)
        if nr is not None:
            kept = count_nodes(nr)
            if kept + sims - 1 <= max_nodes:
                return nr, kept
    return Node(state, rules), 0


def find(dump, s0, s1, turn):
    """advance() on a dump: the id of the node to re-root at, or None."""
    def holds(i):
        return (int(dump["s0"][i]), int(dump["s1"][i]), int(dump["turn"][i])) == (s0, s1, turn)

    def children(i):
        return [int(c) for c in dump["child"][i][: int(dump["nmoves"][i])] if int(c) != 0xFFFF]

    hit = next((c for c in children(0) if holds(c)), None)
    if hit is None:
        hit = next((g for c in children(0) for g in children(c) if holds(g)), None)
    if hit is None or not int(dump["evaluated"][hit]) or int(dump["nmoves"][hit]) == 0:
        return None
    return hit


def compact(dump, new_root):
    """The dump (numpy records, _native.C4_PNODE_DTYPE) that the re-root at node `new_root`
    must leave: the nodes of its subtree in increasing old id, renumbered from 0; parents and
    children renumbered, the new root without parent, depths counted from it; every other
    field as it was."""
    remap = {}
    for i in range(len(dump)):
        if i == new_root or int(dump["parent"][i]) in remap:
            remap[i] = len(remap)
    old = sorted(remap)
    out = dump[old].copy()
    d0 = int(dump["depth"][new_root])
    for new, o in enumerate(old):
        if new == 0:
            out["parent"][new], out["pact"][new], out["depth"][new] = 0xFFFF, 0xFF, 0
        else:
            out["parent"][new] = remap[int(dump["parent"][o])]
            out["depth"][new] = int(dump["depth"][o]) - d0
        for k in range(8):
            ch = int(dump["child"][o][k])
            if ch != 0xFFFF:
                out["child"][new][k] = remap[ch]   # a kept node's children are all kept
    return out
