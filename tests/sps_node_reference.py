"""Numpy restatement of what the reference's two SPS nodes do with the scores of a frame
(c_ws/src/sps_filter/scripts/sps_node.py:123-161, sps_node_cvm.py:145-184): the checker of sps_filter_finish and of
sps_amd.sps_filters.  No GPU needed to import."""
import numpy as np


def finish_reference(scores, raw, batch, n_sub, eps, keep_strict, label_col=3):
    """scores [n] f32; raw [n, cols] f32 rows as received; batch [>= n + n_sub, 5] f32 rows of sps_filter_prepare.
    Returns dict(filtered, labels, cloud_tr, submap, sums): sums = [count, TP, FP, FN, TN, sum (s-g)^2, sum g, sum g^2]
    in float64 (None without a label column)."""
    s = np.asarray(scores, dtype=np.float32)
    raw = np.asarray(raw, dtype=np.float32)
    n = len(s)
    e = np.float32(eps)
    with np.errstate(invalid="ignore"):
        pred = np.where(s < e, 0, 1)                                      # sps_node.py:131 (a NaN score gives 1)
        keep = (pred == 0) if keep_strict else (s <= e)                   # sps_node_cvm.py:171 / sps_node.py:148
    out = dict(filtered=raw[keep], labels=pred.astype(np.int32),
               cloud_tr=np.hstack([batch[:n, 1:4], pred.reshape(-1, 1).astype(np.float32)]).astype(np.float32),   # :153
               submap=np.hstack([batch[n:n + n_sub, 1:4], np.ones((n_sub, 1), np.float32)]).astype(np.float32),   # :157-160
               sums=None)
    if label_col is not None and raw.shape[1] > label_col:
        g = raw[:, label_col]
        with np.errstate(invalid="ignore"):
            gt = np.where(g < e, 0, 1)                                    # :132
        s64, g64 = s.astype(np.float64), g.astype(np.float64)
        out["sums"] = np.array([n, ((gt == 1) & (pred == 1)).sum(), ((gt == 0) & (pred == 1)).sum(),
                                ((gt == 1) & (pred == 0)).sum(), ((gt == 0) & (pred == 0)).sum(),
                                ((s64 - g64) ** 2).sum(), g64.sum(), (g64 * g64).sum()], dtype=np.float64)
    return out


def sums_from_labels(gt, pred):
    """An accumulator row whose confusion counts are those of two 0 / 1 label vectors (the regression sums zero)."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    return [len(gt), ((gt == 1) & (pred == 1)).sum(), ((gt == 0) & (pred == 1)).sum(), ((gt == 1) & (pred == 0)).sum(),
            ((gt == 0) & (pred == 0)).sum(), 0.0, 0.0, 0.0]
