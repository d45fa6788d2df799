"""numpy restatements for the diffusion-classifier tests, written from the definition (classify.py's module text) with
plain loops and not imported from the package:

    score[i, c] = sum_l w_l * mean_d se[d, l, i, c] / CHW,   pred[i] = argmin_c (a tie to the lower index),
    margin[i]   = second-lowest score - lowest score."""
import math

import numpy as np


def class_weights(sigmas, weighting, sigma_data):
    out = []
    for s in sigmas:
        if weighting == "edm":
            out.append((s ** 2 + sigma_data ** 2) / (s ** 2 * sigma_data ** 2))
        elif weighting == "eps":
            out.append(1.0 / s ** 2)
        elif weighting == "uniform":
            out.append(1.0)
        else:
            raise ValueError(weighting)
    return np.array(out, dtype=np.float64)


def class_scores(se, chw, weights):
    R, L, n, C = se.shape
    out = np.zeros((n, C), dtype=np.float64)
    for i in range(n):
        for c in range(C):
            acc = 0.0
            for l in range(L):
                acc += weights[l] * (sum(se[d, l, i, c] for d in range(R)) / R) / chw
            out[i, c] = acc
    return out


def _lowest(row):
    """(index of the lowest value, the first of equals; second-lowest - lowest)"""
    best = 0
    for c in range(1, len(row)):
        if row[c] < row[best]:
            best = c
    rest = [row[c] for c in range(len(row)) if c != best]
    return best, (min(rest) - row[best] if rest else math.inf)


def predict(scores):
    got = [_lowest(list(row)) for row in scores]
    return np.array([g[0] for g in got], dtype=np.int64), np.array([g[1] for g in got], dtype=np.float64)


def level_predictions(se):
    R, L, n, C = se.shape
    out = np.zeros((L, n), dtype=np.int64)
    for l in range(L):
        for i in range(n):
            out[l, i] = _lowest([sum(se[d, l, i, c] for d in range(R)) / R for c in range(C)])[0]
    return out


def confusion_matrix(pred, labels, C):
    out = np.zeros((C, C), dtype=np.int64)
    for p, t in zip(pred, labels):
        out[int(t), int(p)] += 1
    return out


def merge_counts(parts):
    out = np.zeros(np.shape(parts[0]), dtype=np.int64)
    for p in parts:
        out += np.asarray(p, dtype=np.int64)
    return out


def classification_stats(confusion):
    m = np.asarray(confusion)
    n = int(m.sum())
    right = sum(int(m[c, c]) for c in range(m.shape[0]))
    a = right / n
    per = []
    for c in range(m.shape[0]):
        k = int(m[c].sum())
        per.append(int(m[c, c]) / k if k else None)
    return {"accuracy": a, "accuracy_stderr": math.sqrt(a * (1 - a) / n) if n >= 2 else None, "per_class_accuracy": per,
            "count": n}
