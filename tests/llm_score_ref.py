"""float64 restatement of ld_llm_token_logprobs and the cases it is tested on (shared by tests/test_gpu_llm_score.py, which runs
the kernel on them, and tests/test_llm_score_host.py, which checks on the CPU that the cases can tell a wrong kernel from a right
one).  Reference: lm_model.py:417-454 and landiff/utils.py:345-359 (top_p_probability), in the log domain."""
import math

import torch

F64 = torch.float64
N_POS = 192            # rows of the schedule tables of every case


def ref_logprob_row(lc, lu, guided, scale, temperature, allowed_ids, forced_id, top_k, top_p, target):
    """One row in float64 from the fp32 inputs -> (logprob, valid).  allowed_ids: the restriction of the position ([] = none)."""
    if forced_id >= 0:
        return 0.0, 0
    l = lc.to(F64)
    if guided:
        u = lu.to(F64)
        l = u + scale * (l - u)
    l = l / temperature
    V = l.numel()
    if allowed_ids:
        mask = torch.full_like(l, -math.inf)
        mask[allowed_ids] = 0.0
        l = l + mask
    elif top_k is not None and 0 < top_k < V:
        thr = torch.topk(l, top_k).values[-1]
        l = l.masked_fill(l < thr, -math.inf)                  # ties at the threshold stay
    if l[target] == -math.inf:
        return -math.inf, 1
    lp = (l[target] - l.max()) - torch.log(torch.exp(l - l.max()).sum())
    if top_p is not None and not allowed_ids:
        p = torch.softmax(l, -1)
        sp, si = torch.sort(p, descending=True, stable=True)   # stable: equal probabilities keep their id order
        cum = torch.cumsum(sp, -1)
        rem = cum >= top_p
        rem[1:] = rem[:-1].clone()
        rem[0] = False
        removed = torch.zeros(V, dtype=torch.bool).scatter(0, si, rem)
        if removed[target]:
            return -math.inf, 1
        lp = lp - torch.log(p[~removed].sum())
    return float(lp), 1


def ref_logprobs(case, *, pos_shift=0, drop_temperature=False, swap_rows=False):
    """All rows of a case -> (logprob float64 [n], valid int [n]).  The keywords are the three wrong kernels the cases must catch:
    the table row of position + 1 + pos_shift, temperature ignored, cond / uncond exchanged."""
    out, val = [], []
    cond, uncond = (case["uncond"], case["cond"]) if swap_rows else (case["cond"], case["uncond"])
    for r in range(case["n"]):
        q = case["positions"][r] + 1 + pos_shift
        al = case["allowed"][q]
        lp, v = ref_logprob_row(cond[r], uncond[r], case["guided"], case["scale"], 1.0 if drop_temperature else case["temperature"],
                                al[1:1 + int(al[0])].tolist(), int(case["forced"][q]), case["top_k"], case["top_p"],
                                int(case["target"][r]))
        out.append(lp); val.append(v)
    return torch.tensor(out, dtype=F64), torch.tensor(val, dtype=torch.int32)


# (guided, temperature, top_k, top_p)
SETTINGS = [(True, 1.0, None, None), (False, 0.7, None, None), (True, 0.7, 5, None), (True, 1.0, 1, None),
            (False, 1.0, None, 0.3), (True, 0.7, None, 0.9), (True, 1.0, 5, 0.9)]
KINDS = ["free", "restricted_in", "free", "restricted_out", "forced"]
# (layout, n): [2][n][V] planes with padded rows, and the decode's [2P][V] pairs with P = 3
SHAPES = [("planes", 1), ("planes", 5), ("planes", 67), ("pairs", 3)]


def make_case(V, layout, n, si, seed):
    """One launch's worth of rows: logits 4 * N(0, 1); row r is of kind KINDS[(r + si) % 5], so every setting meets free,
    restricted (1-3 allowed ids, target inside / outside) and forced positions; even settings give the position as base + row,
    odd ones as one device word per row (distinct, out of order) with bias -1.  Targets of free rows alternate between one of the
    four most likely ids (finite under the filters) and a random id (mostly removed by them); with top_k = 5 every fourth row has
    its 5th and 6th largest logits equal and the 6th as its target: a tie at the threshold, which must stay."""
    guided, temperature, top_k, top_p = SETTINGS[si]
    g = torch.Generator().manual_seed(seed)
    cond = 4 * torch.randn(n, V, generator=g)
    uncond = 4 * torch.randn(n, V, generator=g)
    scale = 7.5
    word_mode = si % 2 == 1
    if word_mode:
        positions = (torch.randperm(N_POS - 8, generator=g)[:n] + 2).tolist()
    else:
        base = 3 + 2 * si
        positions = [base + r for r in range(n)]
    allowed = torch.zeros(N_POS, 4, dtype=torch.int32)
    forced = torch.full((N_POS,), -1, dtype=torch.int32)
    target = torch.zeros(n, dtype=torch.int64)
    kinds = []
    for r in range(n):
        kind = KINDS[(r + si) % 5]
        kinds.append(kind)
        q = positions[r] + 1
        final = (uncond[r].double() + scale * (cond[r].double() - uncond[r].double())) if guided else cond[r].double()
        order = torch.argsort(final, descending=True)
        if kind == "forced":
            forced[q] = int(torch.randint(0, V, (1,), generator=g))
            target[r] = int(torch.randint(0, V, (1,), generator=g))
        elif kind.startswith("restricted"):
            k = 1 + (r % 3)
            ids = torch.randperm(V, generator=g)[:k + 1]
            allowed[q, 0] = k
            allowed[q, 1:1 + k] = ids[:k].to(torch.int32)
            target[r] = int(ids[r % k]) if kind == "restricted_in" else int(ids[k])
        else:
            if top_k == 5 and r % 4 == 0:
                i5, i6 = int(order[4]), int(order[5])
                cond[r, i6], uncond[r, i6] = cond[r, i5], uncond[r, i5]
                target[r] = i6
            elif r % 2 == 0:
                target[r] = int(order[(r // 2) % 4])
            else:
                target[r] = int(torch.randint(0, V, (1,), generator=g))
    return dict(V=V, layout=layout, n=n, si=si, guided=guided, scale=scale, temperature=temperature, top_k=top_k, top_p=top_p,
                cond=cond, uncond=uncond, positions=positions, word_mode=word_mode, allowed=allowed, forced=forced, target=target,
                kinds=kinds)


def all_cases():
    cases = []
    for vi, V in enumerate((71, 2055)):
        for hi, (layout, n) in enumerate(SHAPES):
            for si in range(len(SETTINGS)):
                cases.append(make_case(V, layout, n, si, seed=1000 * vi + 100 * hi + si))
    return cases


def underflow_case(V):
    """Two unguided rows at temperature 1 whose target sits 200 below the row's maximum: its probability, exp(-200) / sum, is 0 in
    fp32 (and a subnormal's neighbour in any exp-domain kernel), its log-probability an ordinary number near -200."""
    g = torch.Generator().manual_seed(77 + V)
    cond = torch.randn(2, V, generator=g)
    target = torch.tensor([3, V - 2], dtype=torch.int64)
    for r in range(2):
        cond[r, target[r]] = cond[r].max() - 200.0 - r
    return dict(V=V, layout="planes", n=2, si=0, guided=False, scale=7.5, temperature=1.0, top_k=None, top_p=None, cond=cond,
                uncond=torch.randn(2, V, generator=g), positions=[5, 6], word_mode=False, allowed=torch.zeros(N_POS, 4, dtype=torch.int32),
                forced=torch.full((N_POS,), -1, dtype=torch.int32), target=target, kinds=["free", "free"])
