#!/usr/bin/env python3
"""Golden run of the reference's training loop (models/chess_value/network.py:75-101 `train`).

Runs ONLY in the build container: imports the reference's network.py by file path
(unmodified) and calls its own `train` on a fixed set — the first N positions of
chess_tensor.json (their recorded state_to_tensor planes), fixed labels, `ValueNetwork(8, 1)`
after torch.manual_seed(SEED), a DataLoader with shuffle=False and batch 16 (so the last batch
is partial), 2 epochs, on the CPU.  Recorded: the per-epoch averages (network.py only prints
them, to 4 digits: a forward hook on the model recomputes every batch's nn.MSELoss from the
very outputs `train` saw, and the averages are summed as :96-98 do), the value `train` returns
(the quirk of :82-101 included) and the final head weights.

The run is made with 1 and with 16 torch threads; the fixture stores the 16-thread run and the
largest relative difference between the two as "thread_rel_diff", the measured run-to-run
spread of the reference itself that tests/test_learner_cpu.py scales its tolerance from.

Usage: python tests/golden/gen_golden_train.py
"""
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ZC_REFERENCE", "/root/reference")
SEED, N, EPOCHS, BATCH, LR = 4321, 40, 2, 16, 1e-3


def labels(n):
    return np.asarray([(i * 7 + 3) % 3 - 1 for i in range(n)], np.float32)


def run(mod, x, y, threads):
    torch.set_num_threads(threads)
    torch.manual_seed(SEED)
    model = mod.ValueNetwork(8, 1)
    loader = torch.utils.data.DataLoader(mod.ValueNetDataset(x, y), batch_size=BATCH, shuffle=False, num_workers=0)
    crit, batch_losses, lo = torch.nn.MSELoss(), [], [0]

    def hook(_m, _inp, out):
        n = out.shape[0]
        t = torch.from_numpy(y[lo[0]:lo[0] + n]).float().unsqueeze(1)
        batch_losses.append((crit(out.detach(), t).item(), n))
        lo[0] = (lo[0] + n) % len(y)
    h = model.register_forward_hook(hook)
    ret = mod.train(model, loader, epochs=EPOCHS, lr=LR, device="cpu")
    h.remove()
    per = (len(y) + BATCH - 1) // BATCH
    epochs = [sum(l * n for l, n in batch_losses[e * per:(e + 1) * per]) / len(y) for e in range(EPOCHS)]
    lin = model.head[2]
    return dict(epoch_losses=epochs, returned=float(ret.detach()), head_weight=[float(v) for v in lin.weight.detach().reshape(-1)],
                head_bias=float(lin.bias.detach().item()))


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def main():
    spec = importlib.util.spec_from_file_location("ref_network", os.path.join(REF, "models/chess_value/network.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(HERE, "chess_tensor.json")) as f:
        cases = json.load(f)["cases"][:N]
    x = np.stack([np.unpackbits(np.frombuffer(bytes.fromhex(c["bits"]), np.uint8))[:17 * 64].reshape(17, 8, 8)
                  for c in cases]).astype(np.float32)
    y = labels(len(cases))
    one, many = run(mod, x, y, 1), run(mod, x, y, 16)
    diff = max(rel(one[k], many[k]) for k in ("epoch_losses", "returned", "head_weight", "head_bias"))
    out = dict(meta=dict(generator="tests/golden/gen_golden_train.py",
                         reference="models/chess_value/network.py train, ValueNetwork(8, 1), CPU", torch=torch.__version__),
               seed=SEED, positions=len(cases), epochs=EPOCHS, batch_size=BATCH, lr=LR, labels=[int(v) for v in y],
               thread_rel_diff=diff, **many)
    with open(os.path.join(HERE, "train_value_c8b1.json"), "w") as f:
        json.dump(out, f)
    print("wrote train_value_c8b1.json", many["epoch_losses"], many["returned"], "thread_rel_diff", diff)


if __name__ == "__main__":
    main()
