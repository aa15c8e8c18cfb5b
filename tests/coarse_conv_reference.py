"""A plain numpy reference of ONE block of the network, from the taps that feed it: float64, or float32 with a chosen
summation order of the kernel offsets.  Pair lists are the oracle's (CoordinateManager.k3 / kdown); nothing else is shared
with it -- tests/test_coarse_conv_cpu.py shows that the float32 form in ascending order reproduces the oracle's taps.

    sparse convolution          out[o] += x[i] @ W[k]          over the pairs (i, o) of every offset k
    stride-2 convolution        the same over kdown(ts): in = fine rows, out = coarse rows
    transposed convolution      the same pairs with in / out swapped
    BN (eval)                   (y - mean) / sqrt(var + 1e-5) * weight + bias
    block                       relu(bn2(conv2(relu(bn1(conv1(x))))) + r),  r = x or bn(x @ W_downsample)

What feeds which block (the taps of sps_get_feature):
    block2 <- conv2p2s2(block1)            block5 <- cat(convtr4p16s2(block4), block3)
    block3 <- conv3p4s2(block2)            block6 <- cat(convtr5p8s2(block5), block2)
    block4 <- conv4p8s2(block3)            block7 <- cat(convtr6p4s2(block6), block1)

The tolerance of a comparison with the device comes from the reference alone (`spread`): the largest difference from float64
of the float32 form summed in ascending, descending and four-contiguous-splits order of the offsets."""
import numpy as np

BN_EPS = 1e-5
ORDERS = ("ascending", "descending", "splits")
#            block: (level, upstream tap, stride-2 conv + its BN | transposed conv + its BN, skip tap)
BLOCKS = {"block2": (2, "block1", ("conv2p2s2", "bn2"), None),
          "block3": (3, "block2", ("conv3p4s2", "bn3"), None),
          "block4": (4, "block3", ("conv4p8s2", "bn4"), None),
          "block5": (3, "block4", ("convtr4p16s2", "bntr4"), "block3"),
          "block6": (2, "block5", ("convtr5p8s2", "bntr5"), "block2"),
          "block7": (1, "block6", ("convtr6p4s2", "bntr6"), "block1")}


def conv(x, n_out, pairs, W, dtype, order="ascending", transpose=False):
    """out[o] += x[i] @ W[k]; `order` = the order in which the offsets' terms meet ("splits": four contiguous runs of the
    offsets that hold pairs, each summed on its own, then added -- the shape of a split-K reduction)."""
    W = np.asarray(W, dtype)
    x = np.asarray(x, dtype)
    ks = [k for k, (i, _) in enumerate(pairs) if len(i)]
    if order == "descending":
        ks = ks[::-1]
    runs = [ks]
    if order == "splits":
        per = -(-len(ks) // 4) if ks else 1
        runs = [ks[j:j + per] for j in range(0, len(ks), per)]
    parts = []
    for run in runs:
        out = np.zeros((n_out, W.shape[2]), dtype)
        for k in run:
            i, o = pairs[k]
            if transpose:
                i, o = o, i
            out[o] += x[i] @ W[k]                      # an output row occurs at most once per offset
        parts.append(out)
    total = parts[0] if parts else np.zeros((n_out, W.shape[2]), dtype)
    for p in parts[1:]:
        total = total + p
    return total


def bn(p, name, y, dtype):
    w, b, mean, var = (np.asarray(p[f"{name}.bn.{s}"], dtype) for s in ("weight", "bias", "running_mean", "running_var"))
    invstd = (dtype(1.0) / np.sqrt(var + dtype(BN_EPS))).astype(dtype)
    return ((y - mean) * invstd * w + b).astype(dtype)


def relu(x):
    return np.maximum(x, x.dtype.type(0))


def basic_block(p, name, x, k3, dtype, order):
    n = len(x)
    y = relu(bn(p, f"{name}.0.norm1", conv(x, n, k3, p[f"{name}.0.conv1.kernel"], dtype, order), dtype))
    y = bn(p, f"{name}.0.norm2", conv(y, n, k3, p[f"{name}.0.conv2.kernel"], dtype, order), dtype)
    ds = f"{name}.0.downsample.0.kernel"
    if ds in p:
        cout = p[f"{name}.0.conv1.kernel"].shape[2]
        r = (x @ np.asarray(p[ds], dtype).reshape(x.shape[1], cout)).astype(dtype)
        r = bn(p, f"{name}.0.downsample.1", r, dtype)
    else:
        r = x
    return relu(y + r)


def block_from_taps(p, cm, taps, block, dtype=np.float64, order="ascending"):
    """Tap `block` [V_level, C] from the taps that feed it (rows in the ORACLE's order: cm.coords), in `dtype`."""
    level, up, (cname, bname), skip = BLOCKS[block]
    ts = 1 << level
    x = np.asarray(taps[up], dtype)
    n = len(cm.coords[ts])
    if skip is None:
        y = conv(x, n, cm.kdown(ts // 2), p[cname + ".kernel"], dtype, order)
    else:
        y = conv(x, n, cm.kdown(ts), p[cname + ".kernel"], dtype, order, transpose=True)
    y = relu(bn(p, bname, y, dtype))
    if skip is not None:
        y = np.concatenate([y, np.asarray(taps[skip], dtype)], axis=1)
    return basic_block(p, block, y, cm.k3(ts), dtype, order)


def spread(p, cm, taps, block, ref=None):
    """max over the three float32 summation orders of max |float32 form - float64 form|."""
    if ref is None:
        ref = block_from_taps(p, cm, taps, block, np.float64)
    return max(float(np.abs(block_from_taps(p, cm, taps, block, np.float32, o).astype(np.float64) - ref).max()) for o in ORDERS)


def bound(spread_value, ref):
    """What a correct kernel may differ from the float64 reference by.  The device sums the same terms in another order, and
    two orders of one sum differ by a small multiple of each other's error: 16 spreads.  A lost or doubled unit is four
    products among at most 81 * 96, each about as large as a term, where the rounding of the whole sum is ~sqrt(T) * 2^-24
    of a term: 10^4 .. 10^6 times above rounding, far beyond the factor.  The floor covers taps whose three float32 forms
    happen to agree."""
    return max(16.0 * spread_value, 1e-6 * float(np.abs(ref).max()))
