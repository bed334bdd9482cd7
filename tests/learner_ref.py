"""Executable spec of the learner's two device steps (include/zeroclone.h, "training"), in
numpy: `batch_ref` is zc_train_batch_async built on selfplay.planes, the chess oracle's move
lists and tensors and the single-precision division of the policy targets; `loss_ref` is
zc_train_loss_async's definition in fp64."""
import numpy as np

C4, CHESS = "c4", "chess"
STRIDE = {C4: 7, CHESS: 256}
WIDTH = {C4: 7, CHESS: 4096}


def chess_row(state: dict) -> np.ndarray:
    """A tests/golden/chess_*.json state as a zc_chess_state row, [9] int64."""
    raw = np.zeros(72, np.uint8)
    raw[:64] = np.frombuffer(state["board"].encode("latin-1"), np.uint8)
    raw[64], raw[65], raw[66] = state["turn"], state["fifty"], state["castle"]
    return raw.view(np.int64).copy()


def logit_index(ids: np.ndarray, width: int) -> np.ndarray:
    ids = ids.astype(np.int64) & 0xFFFF
    return ids if width == 7 else (ids & 63) * 64 + ((ids >> 6) & 63)


def _chess_lists(row: np.ndarray):
    """(planes [17, 8, 8], packed legal moves) of one zc_chess_state row, by the chess oracle."""
    import oracle
    from zeroclone_amd import _native
    raw = row.view(np.uint8)
    s = oracle.chess_state(raw[:64].tobytes().decode("latin-1"), int(raw[64]), int(raw[65]), int(raw[66]))
    if oracle.chess_move_count(s) > STRIDE[CHESS]:   # status bit 2: no list
        return oracle.chess_tensor(s), None
    moves = [_native.pack_chess_move(fr, fc, tr, tc, val) for fr, fc, tr, tc, val in oracle.chess_moves(s)]
    return oracle.chess_tensor(s), moves


def batch_ref(game: str, rows: np.ndarray, labels: np.ndarray, pi_off, pi, index, flags=None) -> dict:
    """zc_train_batch_async: batch row b = set row index[b].  rows [n, 3 | 9] int64, labels [n],
    pi_off [n + 1] / pi (the TrajBatch CSR; None: no policy), flags [B] (bit 0: mirror) or None."""
    from zeroclone_amd import selfplay
    index = np.asarray(index, np.int64)
    B, stride = len(index), STRIDE[game]
    out = dict(planes=np.zeros((B, 2, 6, 7) if game == C4 else (B, 17, 8, 8), np.float32),
               z=labels[index].astype(np.float32), legal=np.zeros((B, stride), np.uint16),
               n_legal=np.zeros(B, np.int32), target=np.zeros((B, stride), np.float32), status=0)
    for b, i in enumerate(index):
        mirror = bool(flags is not None and int(flags[b]) & 1)
        if game == C4:
            p = selfplay.planes(rows[i:i + 1])[0]
            occ = int(rows[i, 0]) | int(rows[i, 1])
            moves = [c for c in range(7) if not (occ >> (7 * c + 5)) & 1]   # in the set's columns
            if mirror:
                p = p[:, :, ::-1]
            out["planes"][b] = p
        else:
            assert not mirror, "a chess position has no mirror image"
            out["planes"][b], moves = _chess_lists(rows[i])
            if moves is None:   # more legal moves than the row holds: n_legal 0, planes and label decoded
                out["status"] |= 4
                moves = []
        ent = [] if pi_off is None else [int(e) & 0xFFFFFFFF for e in pi[int(pi_off[i]):int(pi_off[i + 1])]]
        total = np.float32(sum(e >> 16 for e in ent))
        key = (lambda m: m) if game == C4 else (lambda m: m & 0xFFF)   # chess: by from / to
        counts = {}
        for e in ent:
            if key(e & 0xFFFF) in [key(m) for m in moves]:
                counts[key(e & 0xFFFF)] = e >> 16
            else:
                out["status"] |= 1   # dropped; its count stays in the sum
        if game == C4 and mirror:
            moves = sorted(6 - c for c in moves)
            counts = {6 - c: k for c, k in counts.items()}
        out["n_legal"][b] = len(moves)
        for j, m in enumerate(moves):
            out["legal"][b, j] = m
            k = counts.get(key(m), 0)
            out["target"][b, j] = np.float32(k) / total if k else np.float32(0)   # one IEEE single division
    return out


def loss_ref(v, logits, z, legal, n_legal, target):
    """zc_train_loss_async in fp64: (Lv, Lp, grad_v [B], grad_logits [B, width] or None).
    logits None: a value-only model.  The header's rules for rows no minibatch holds: n_legal is
    clamped to [0, stride]; a width-7 id above 6 names no logit and is ignored, in the softmax and
    in the target sum alike; a policy row is one whose legal slots' targets (the slots below the
    clamped n_legal whose id is not ignored) sum to more than 0."""
    v, z = np.asarray(v, np.float64).reshape(-1), np.asarray(z, np.float64)
    B = len(v)
    Lv = float(np.mean((v - z) ** 2))
    grad_v = 2.0 * (v - z) / B
    if logits is None:
        return Lv, 0.0, grad_v, None
    x = np.asarray(logits, np.float64)
    width = x.shape[1]
    t = np.asarray(target, np.float64)
    stride = t.shape[1]

    def slots(b):
        """The legal slots of row b that name a logit, and those logits' indices."""
        n = min(max(int(n_legal[b]), 0), stride)
        idx = logit_index(np.asarray(legal[b, :n]), width)
        keep = np.flatnonzero(idx < width)
        return keep, idx[keep]
    policy = [b for b in range(B) if t[b, slots(b)[0]].sum() > 0]
    P = len(policy)
    grad = np.zeros_like(x)
    Lp = 0.0
    for b in policy:
        at, idx = slots(b)
        xs = x[b, idx]
        m = xs.max()
        e = np.exp(xs - m)
        logp = (xs - m) - np.log(e.sum())
        Lp += -(t[b, at] * logp).sum() / P
        grad[b, idx] = (e / e.sum() - t[b, at]) / P
    return Lv, Lp, grad_v, grad


def hand_made_rule_rows(seed=21):
    """Eight width-7, stride-7 rows that no minibatch holds, one per rule of zc_train_loss_async's
    header: rows 0-2 carry an id of 7, 63 and 0xFFFF in a legal slot with a target (ignored: row
    0's list also holds column 6, which a clamp would count twice); row 3 has targets past n_legal
    only and row 5 on an ignored id only (no policy rows); row 6 has n_legal -3 (no legal slot,
    no policy row), row 7 n_legal stride + 5 (all 7 slots).  The targets are dyadic and sum to 1
    over the slots that count, where (p - t) / P is also autograd's gradient."""
    g = np.random.default_rng(seed)
    nl = np.asarray([4, 3, 5, 2, 7, 3, 2, 4], np.int32)
    legal, target = np.zeros((8, 7), np.uint16), np.zeros((8, 7), np.float32)
    for b in range(8):
        legal[b, :nl[b]] = np.sort(g.choice(7, nl[b], replace=False))
    legal[0, :4], target[0, :4] = [2, 7, 5, 6], [0.25, 0.25, 0.25, 0.5]
    legal[1, 1], target[1, :3] = 63, [0.5, 0.5, 0.5]
    legal[2, 1], target[2, :5] = 0xFFFF, [0.25] * 5
    target[3, 4] = 0.5
    target[4, :7] = [0.125, 0.125, 0.25, 0, 0.25, 0.125, 0.125]
    legal[5, :3], target[5, 1] = [1, 9, 4], 1.0
    target[6, :2] = [0.5, 0.5]
    nl[6], nl[7] = -3, 12
    legal[7], target[7] = np.arange(7), [0.125] * 6 + [0.25]
    return dict(v=np.tanh(g.normal(size=8)), z=g.integers(-1, 2, 8).astype(np.float32),
                logits=g.normal(size=(8, 7)) * 2.0, legal=legal, n_legal=nl, target=target)
