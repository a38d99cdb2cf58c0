"""tests/logistic_bound.py is worth something on the TOPICS' hard inputs (CPU): for every hostile and every width case of
tests/topics_hard_cases.py -- exactly what tests/test_gpu_topics_hard.py steps -- and EVERY topic, the honest fp32 emulation of the single
model on (csr, plane t) stays inside dw, dloss and dc; the mistakes that only several topics side by side can make leave dw:

  label_from_neighbour   topic t reads plane t ^ 1
  weight_from_neighbour  topic t's dot uses W[t ^ 1]
  word_to_neighbour      topic t's sums land on word t ^ 1 (the finish of topic t reads what topic t ^ 1 added)
  pad_not_zero           a padding topic's coefficient (weight 0, label +1: c = -1/2) is added to the last real topic's word
  fold_head              logistic_bound's fold_2048 at the form's own head: the first rank beyond the head (n_hot) lands on its last word
  head_beyond_dp         a narrow model's head flush over all n_hot * tp words, the words at j >= dp * tp not zero (modelled: the head's
                         own words again, modulo dp ranks): those beyond the worker's block of acc_stride(dp) ranks land in the NEXT
                         worker's block.  Applies where n_hot > acc_stride(dp) and K > 1 -- not at wide 128, whose head of 32 ranks
                         ends with the block of the narrowest model (asserted)
  vexp_qscale, vexp_finish   logistic_bound's own

NAMED says on which case, form, topic and step each must leave the bound.  These model, on the CPU, the reverts the GPU module is there to
catch: a head size off by one rank IS fold_head (one rank more: the first rank beyond is indexed into the next word of LDS, the head's
flush lands it one rank off) at dim = n_hot, where test_width_edges' named ranks n_hot - 1 and n_hot carry data; the wide scatter's at[1]
written to at[0] is word_to_neighbour on the odd topics; vexp + 1 in qscale is vexp_qscale.  (A finish that zeroes only ap[0] leaves a
step's own result right and the NEXT step wrong by the stale sums of topics t0 + 2 and t0 + 3, at full scale in the exact cases: no
one-step emulation models it; the GPU module's list step behind every step does.)

The exact cases' expectations are computed and held against the fp64 reference where they are built (topics_hard_cases.exact_case through
logistic_hard_cases.exact_step); test_exact_cases_are_exact builds every one and checks the scale and the signs they reach.
"""

import functools

import numpy as np
import pytest

import logistic_bound as lb
import logistic_hard_cases as lhc
import logistic_ref as ref
import topics_hard_cases as tc
from test_logistic_hard_bound import FLOAT_PRECISION

THREE, RANGES_H, RANGES_W = "3 workers 100/37/1", "ranges 1500/547/1", "ranges 300/299/1"
# mutation -> group -> [(case name, form, T, topic, step)]
NAMED = {
    "label_from_neighbour": {"hostile": [("signed", "wide", 128, 4, THREE)], "width": [("dim 64", "interleaved", 32, 4, THREE)]},
    "weight_from_neighbour": {"hostile": [("signed", "wide", 128, 5, THREE), ("signed", "wide", 128, 0, THREE)], "width": [("dim 64", "interleaved", 32, 5, THREE)]},
    "word_to_neighbour": {"hostile": [("ragged64", "wide", 128, 127, THREE), ("signed", "planar", 8, 0, THREE)], "width": [("dim 32", "wide", 128, 127, RANGES_W)]},
    "pad_not_zero": {"hostile": [("wide", "wide", 33, 32, THREE), ("ragged64", "wide", 103, 102, RANGES_H)],
                     "width": [("dim 39", "wide", 103, 102, THREE), ("dim 170", "interleaved", 9, 8, THREE)]},
    "fold_head": {"hostile": [("wide", f, T, T - 1, RANGES_H) for f, T in tc.H_FORMS["wide"]],
                  "width": [("dim %d" % tc.N_HOT[ft], ft[0], ft[1], ft[1] - 1, step) for ft in tc.W_SETS for step in (THREE, RANGES_W)]},
    "head_beyond_dp": {"width": [("dim 1", f, T, T - 1, step) for f, T in tc.W_SETS if (f, T) != ("wide", 128) for step in (THREE, RANGES_W)] +
                                [("dim 62", "planar", 8, 7, THREE)]},
    # (scaled_m30's dense topics have weights near 2^30 on values near 2^-30: a step moves them by less than their own rounding, and
    #  half a gradient hides there.  Topic 0 carries the trait's own weights, as the single model's case does.)
    "vexp_qscale": {"hostile": [("scaled_m30", "wide", 128, 0, THREE)], "width": [("dim 1", "wide", 128, 65, THREE)]},
    "vexp_finish": {"hostile": [("scaled_p10", "interleaved", 32, 31, THREE), ("scaled_p10", "planar", 8, 0, THREE)],
                    "width": [("dim 256", "planar", 8, 3, "ranges k16 x 37")]},
}
# One step's bound is float precision: max(bound) < FLOAT_PRECISION max |want|, the single model's ratio.  Two kinds of case have a ratio of
# their own, both for tests/test_softmax_bound.py's reason: the step lr G outweighs the weights it starts from, max |want| is then the
# GRADIENT's size and the ratio the gradient's relative bound, dc_i = dz_i / 4 + ... against coefficients of order 1.  On scaled_p10 (values
# 2^10 times the base's, dense topics of logit scale 2, rows of up to 13 chunks) dc_i reaches 2e-5, as it does for softmax's dense classes.
# On the hand-built width rows beyond 64 keys (dim 111 .. 254: up to dim + 1 entries of magnitude up to 2, not normalised, 300 of them
# summed by one worker) sum_j |x_ij| |w_j| is many times the logit and gamma(m_i + 4) grows with the row's 7 to 16 chunks.
OWN_PRECISION = {("hostile", "scaled_p10"): 5e-5}
OWN_PRECISION.update({("width", d): 3e-5 for d in (111, 112, 113, 126, 127, 128, 168, 169, 170, 254)})
RATIOS = {}


def key_of(group, name):
    return (group, name if group == "hostile" else int(name.split()[1]))


def all_dots(case, t):
    """the emulated fp32 dot of every row of topic t"""
    return lb.emu_dots(tc.topic_csr(case, t), case.W[t], np.arange(len(case.csr[3])))


def applies(mut, case, form, T, t, lists):
    dp = case.dim + 1
    if mut in ("label_from_neighbour", "weight_from_neighbour", "word_to_neighbour"):
        return (t ^ 1) < T
    if mut == "pad_not_zero":
        return tc.tp_of(form, T) > T and t == T - 1
    if mut == "fold_head":
        return dp > tc.n_hot(form, T)
    if mut == "head_beyond_dp":
        return len(lists) > 1 and dp < tc.n_hot(form, T) and tc.n_hot(form, T) > tc.acc_stride(dp)
    return True


def mutated_step(case, form, T, t, name, mut):
    """float32 [dp]: topic t's weights after the step under the mutation, emulated"""
    lists, lr = tc.step_cases(case)[name]
    csr, w, dp, u = tc.topic_csr(case, t), case.W[t], case.dim + 1, t ^ 1
    assert applies(mut, case, form, T, t, lists), (mut, case.name, form, T, t)
    if mut == "label_from_neighbour":
        return lb.emu_step(tc.topic_csr(case, u), w, lists, lr, case.lam, d=all_dots(case, t))
    if mut == "weight_from_neighbour":
        return lb.emu_step(csr, w, lists, lr, case.lam, d=all_dots(case, u))
    if mut in ("vexp_qscale", "vexp_finish"):
        return lb.emu_step(csr, w, lists, lr, case.lam, mut, d=all_dots(case, t))
    if mut == "word_to_neighbour":
        accs = [lb.emu_acc(tc.topic_csr(case, u), case.W[u], idx, d=all_dots(case, u)) for idx in lists]
        return lb.emu_finish(csr, w, accs, lr, case.lam)
    d = all_dots(case, t)
    if mut == "fold_head":
        return lb.emu_finish(csr, w, [lb.emu_acc(csr, w, idx, "fold_2048", d=d, n_hot=tc.n_hot(form, T)) for idx in lists], lr, case.lam)
    accs = [lb.emu_acc(csr, w, idx, d=d) for idx in lists]
    if mut == "pad_not_zero":   # the padding topic: weight 0 (d = 0) and label +1 on every row
        pad = (case.csr[0], case.csr[1], case.csr[2], np.ones(len(case.csr[3]), np.int8))
        zero = {r: np.float32(0.0) for r in range(len(case.csr[3]))}
        accs = [(acc + lb.emu_acc(pad, np.zeros(dp, np.float32), idx, d=zero)[0], S) for (acc, S), idx in zip(accs, lists)]
    elif mut == "head_beyond_dp":
        key_at = np.argsort(lb.ranks_of(case.csr, dp))   # rank -> key
        stride, out = tc.acc_stride(dp), [acc.copy() for acc, _ in accs]
        for k in range(len(accs) - 1):
            for q in range(stride, tc.n_hot(form, T)):   # head word (rank q) holds rank q % dp's sum; it lands on rank q - stride of worker k + 1
                if q - stride < dp:
                    out[k + 1][key_at[q - stride]] += accs[k][0][key_at[q % dp]]
        accs = [(o, S) for o, (_, S) in zip(out, accs)]
    else:
        raise ValueError(mut)
    return lb.emu_finish(csr, w, accs, lr, case.lam)


@functools.lru_cache(maxsize=None)
def survey(key):
    """One data set, every topic emulated once: {t: (step ratios {name: error / bound}, largest dc ratio, loss ratios {(a, b): .},
    float-precision ratios {name: max bound / max |want|}, uncertain rows {(a, b): count})}"""
    case = tc.bound_case(key)
    out = {}
    for t in range(case.T):
        csr, w, r = tc.topic_csr(case, t), case.W[t], tc.reference(case, t)
        d = all_dots(case, t)
        steps, precision = {}, {}
        for name, (lists, lr) in tc.step_cases(case).items():
            want, bound = r.steps[name]
            got = lb.emu_step(csr, w, lists, lr, case.lam, d=d).astype(np.float64)
            steps[name] = float(np.max(np.abs(got - want) / bound))
            precision[name] = float(np.max(bound)) / float(np.max(np.abs(want)))
        d32 = np.asarray([d[i] for i in range(len(r.d))], dtype=np.float64)
        y = case.P[t].astype(np.float64)
        c_ratio = float(np.max(np.abs(ref.coef(d32, y) - ref.coef(r.d, y)) / lb.dc(r.dz)))
        losses = {}
        for (a, b), (loss, dloss, _, _) in r.evals.items():
            w64 = w.astype(np.float64)
            emu = case.lam * float(np.dot(w64, w64)) + float(np.mean(ref.row_loss(d32[a:b], y[a:b])))
            losses[(a, b)] = abs(emu - loss) / dloss
        out[t] = (steps, c_ratio, losses, precision, {ab: v[3] for ab, v in r.evals.items()})
    tc.forget(case)
    return out


@pytest.mark.parametrize("key", tc.BOUND_KEYS, ids=tc.BOUND_IDS)
def test_emulation_inside_dw_dloss_and_dc(key):
    case, s = tc.bound_case(key), survey(key)
    assert sorted(s) == list(range(case.T)) and case.T >= max(T for _, T in tc.forms_of(key))
    for t, (steps, c_ratio, losses, _, _) in s.items():
        assert set(steps) == set(tc.step_cases(case))
        for name, ratio in steps.items():
            assert ratio <= 1.0, ("dw", t, name, ratio)
        assert c_ratio <= 1.0, ("dc", t, c_ratio)
        for ab, ratio in losses.items():
            assert ratio <= 1.0, ("dloss", t, ab, ratio)
    worst = {"dw": max(max(v[0].values()) for v in s.values()), "dc": max(v[1] for v in s.values()), "dloss": max(max(v[2].values()) for v in s.values())}
    for what, ratio in worst.items():
        RATIOS[(what, key[0])] = max(RATIOS.get((what, key[0]), 0.0), ratio)
    print("%s %s, %d topics: largest emulated error / bound: dw %.6f, dc %.6f, dloss %.6f" % (case.group, case.name, case.T, worst["dw"], worst["dc"], worst["dloss"]))
    print("so far, per group: %s" % {k: round(v, 6) for k, v in sorted(RATIOS.items())})


@pytest.mark.parametrize("key", tc.BOUND_KEYS, ids=tc.BOUND_IDS)
def test_uncertain_rows_and_float_precision(key):
    case, s = tc.bound_case(key), survey(key)
    for a, b in case.evals:
        counts = [s[t][4][(a, b)] for t in range(case.T)]
        print("%s %s [%d, %d): uncertain rows, worst topic %d (topic %d), all topics %d" % (case.group, case.name, a, b, max(counts), int(np.argmax(counts)), sum(counts)))
        assert max(counts) <= 0.01 * (b - a), (a, b, int(np.argmax(counts)), max(counts))
    worst = max((ratio, t, name) for t in s for name, ratio in s[t][3].items())
    print("%s %s: largest max bound / max |want| %.3e (topic %d, %s)" % (case.group, case.name, worst[0], worst[1], worst[2]))
    assert worst[0] < OWN_PRECISION.get(key, FLOAT_PRECISION), worst


@pytest.mark.parametrize("mut", list(NAMED))
def test_topic_level_mutations_leave_the_bound_on_the_named_cases(mut):
    for group, named in NAMED[mut].items():
        for case_name, form, T, t, name in named:
            key = key_of(group, case_name)
            case = tc.bound_case(key)
            assert (form, T) in tc.forms_of(key), (case_name, form, T)
            want, bound = tc.reference(case, t).steps[name]
            ratio = float(np.max(np.abs(mutated_step(case, form, T, t, name, mut).astype(np.float64) - want) / bound))
            print("%-21s %-7s leaves the bound on %s, %s T = %d, topic %d, %s: error / bound %.3g" % (mut, group, case_name, form, T, t, name, ratio))
            assert ratio > 1.0, (mut, case_name, form, T, t, name, ratio)
            tc.forget(case)
    if mut == "head_beyond_dp":   # the one form it cannot touch: the head of 32 ranks ends where the narrowest model's block does
        assert not applies(mut, tc.width(1), "wide", 128, 127, tc.width(1).step[0]) and tc.n_hot("wide", 128) == tc.acc_stride(2)
        assert not any(applies(mut, tc.hostile(t), f, T, 0, tc.hostile(t).step[0]) for t in ("signed",) for f, T in tc.H_FORMS[t])
    if mut == "pad_not_zero":     # no padding topic where T is a multiple of four, none at all in the planar form
        assert not applies(mut, tc.width(1), "planar", 3, 2, None) and not applies(mut, tc.width(1), "wide", 128, 127, None)


@pytest.mark.parametrize("key", tc.EXACT_KEYS, ids=tc.EXACT_IDS)
def test_exact_cases_are_exact(key):
    """exact_case holds every expectation against the fp64 reference; here: the scale the sums reach, on adjacent words"""
    case = tc.exact_case(*key)
    S = lb.shift(case.n)
    sums = [int(v) for v in case.expect.sums]
    top = max(abs(v) for v in sums) << (S - lb.vexp_of(case.csr[2]))   # in units of 2^-23: Python integers
    assert top <= 2 ** 62 << lhc.E_UNIT
    if case.n in (4096, 64) and case.vmax == 1.0 and case.labels == "plus":
        assert top == 2 ** 62 << lhc.E_UNIT          # the accumulator's whole range ...
        j = int(np.argmax(np.abs(case.expect.sums)))
        words = [int(case.signs[t]) * sums[j] << (S - lb.vexp_of(case.csr[2])) for t in range(case.T)]
        assert {abs(x) for x in words} == {top}
        if key[-1] == "alt":                          # ... +2^62 and -2^62 in every pair of adjacent words
            assert all(words[t] == -words[t + 1] for t in range(case.T - 1))
        else:                                         # ... and five equal words across the quad 3 | 4 and the pairs 3 | 4, 5 | 6
            assert words[3] == words[4] == words[5] == words[6] == words[7] == -words[2] and (case.T == 8 or words[8] == -words[7])
    if case.shape == "tall" and case.labels == "alt":
        assert sums[lhc.E_F] == 0 and not np.signbit(case.expect.whole[0][:, lhc.E_F]).any() and np.all(case.expect.whole[1][:, lhc.E_F] == 0.0)
    if "3 workers 4096/64/1" in case.expect.step:
        assert [lb.shift(len(a)) for a in case.expect.step["3 workers 4096/64/1"][0]] == [50, 56, 62]
    for W in case.expect.whole:   # topic t's expectation IS the single model's times s_t
        assert np.array_equal(W, case.signs[:, None].astype(np.float32) * W[0][None])
    if case.shape == "broad":     # the 2,100 shared columns cross every head at full scale
        ranks = lb.ranks_of(case.csr, case.dim + 1)
        beyond = np.where((ranks >= tc.n_hot(case.form, case.T)) & (ranks < lhc.E_BROAD))[0]
        assert len(beyond) == lhc.E_BROAD - tc.n_hot(case.form, case.T) and np.all(np.abs(case.expect.sums[beyond]) == np.abs(case.expect.sums[1]))


@pytest.mark.parametrize("key", tc.W_KEYS, ids=["dim-%d" % k[1] for k in tc.W_KEYS])
def test_edge_ranks_carry_data(key):
    """the premise of the GPU module's edge checks (test_logistic_hard_bound.test_edge_ranks_carry_data's, per topic): the columns on the
    heads' and the tiles' edges have entries, and in every topic their data sums over the whole set stand far above dg"""
    case = tc.width(key[1])
    dp = case.dim + 1
    everything = np.arange(lhc.W_ROWS)
    ranks = lb.ranks_of(case.csr, dp)
    count = np.bincount(case.csr[1], minlength=dp)
    named = sorted({r for form, T in tc.forms_of(key) for r in tc.W_EDGE_RANKS.get((form, T, case.dim), [])})
    assert named or case.dim == 1
    for t in range(case.T if named else 0):
        data = ref.data_sum(tc.topic_csr(case, t), case.W[t], everything)[0]
        bound = lb.dg(tc.topic_csr(case, t), case.W[t], everything, case.lam)
        for r in named:
            k = int(np.where(ranks == r)[0][0])
            assert count[k] > 0 and abs(data[k]) > 4.0 * bound[k], (t, r, k, count[k], data[k], bound[k])
