"""A frozen graph of the SHAPE of the reference's missing MobileNetV2 files (facerec_test.py:216-217, :336-340) -- test infrastructure.

Those files are keras_applications' `MobileNetV2(alpha, input_shape=(size, size, 3), include_top=False, pooling='avg')` frozen:
`Conv1` (3 x 3 / 2) -> `expanded_conv` (no expansion) -> `block_1 ... block_16` (the standard (t, c, n, s) table, widths from
`_make_divisible(c * alpha, 8)`) -> `Conv_1` (1 x 1 to `_make_divisible(1280 * alpha, 8)` above alpha 1, else 1280) -> the global
average pool.  BatchNormalization has epsilon 1e-3, activations are Relu6, a block whose input and output widths agree at stride 1
ends in an Add.  Keras writes `Conv1` and every stride-2 depthwise as ZeroPadding2D(correct_pad) + a VALID convolution: ((0, 1), (0, 1))
on an even map, ((1, 1), (1, 1)) on an odd one (style="keras"); TF-slim exports of the same network say SAME (style="slim").

The weights are seeded.  The BatchNorm behind every linear projection is damped (gamma * 0.4, as tests/mini_resnet_graph.py damps its
increase layers), so the sums down a chain of residual blocks neither explode nor vanish.
"""
import numpy as np

import gb

EPS = 1e-3
# (expansion t, channels c, repeats n, stride s) of blocks 0 .. 16
TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def make_divisible(v, divisor=8, min_value=None):
    min_value = divisor if min_value is None else min_value
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def correct_pad(size, kernel=3):
    adjust = 1 - size % 2
    return (kernel // 2 - adjust, kernel // 2)


def block_table(alpha, blocks=None):
    """[(block id, expansion, output width, stride)], cut to the first `blocks` entries."""
    rows = []
    for t, c, n, s in TABLE:
        for i in range(n):
            rows.append((len(rows), t, make_divisible(int(c * alpha), 8), s if i == 0 else 1))
    return rows if blocks is None else rows[:blocks]


def last_width(alpha):
    return make_divisible(1280 * alpha, 8) if alpha > 1.0 else 1280


def build(alpha=1.0, size=192, seed=0, style="keras", blocks=None, bn="fused", output="global_average_pooling2d_1/Mean"):
    """Serialized GraphDef: input_1 [-1, size, size, 3] -> `output` [-1, last width].  Returns (bytes, info) with
    info = {"widths": [...], "block_outputs": [tensor names], "features": last width, "learning_phase": placeholder name or None}.
    bn: "fused" = FusedBatchNorm (is_training False), "switch" = un-folded arithmetic behind a learning-phase Switch / Merge."""
    assert style in ("keras", "slim") and bn in ("fused", "switch")
    rs = np.random.RandomState(seed)
    b = gb.GraphBuilder()
    b.placeholder("input_1", [-1, size, size, 3])
    phase = "bn_Conv1/keras_learning_phase" if bn == "switch" else None
    if phase:
        b.placeholder(phase, None, dtype=10)

    def batchnorm(name, src, c, damp=1.0):
        g = (damp * rs.uniform(0.8, 1.2, c)).astype(np.float32)
        be = (0.1 * rs.randn(c)).astype(np.float32)
        mu = (0.1 * rs.randn(c)).astype(np.float32)
        var = rs.uniform(0.5, 1.5, c).astype(np.float32)
        for nm, v in (("gamma", g), ("beta", be), ("moving_mean", mu), ("moving_variance", var)):
            b.const("%s/%s" % (name, nm), v)
        ins = ["%s/%s" % (name, nm) for nm in ("gamma", "beta", "moving_mean", "moving_variance")]
        if bn == "fused":
            b.node(name + "/FusedBatchNorm_1", "FusedBatchNorm", [src] + ins, epsilon=EPS, is_training=False, data_format="NHWC")
            return name + "/FusedBatchNorm_1"
        b.const(name + "/batchnorm/add/y", np.float32(EPS))
        b.node(name + "/cond/Switch_1", "Switch", [src, phase])
        b.node(name + "/batchnorm/add", "Add", [ins[3], name + "/batchnorm/add/y"])
        b.node(name + "/batchnorm/Rsqrt", "Rsqrt", [name + "/batchnorm/add"])
        b.node(name + "/batchnorm/mul", "Mul", [name + "/batchnorm/Rsqrt", ins[0]])
        b.node(name + "/batchnorm/mul_1", "Mul", [name + "/cond/Switch_1", name + "/batchnorm/mul"])
        b.node(name + "/batchnorm/mul_2", "Mul", [ins[2], name + "/batchnorm/mul"])
        b.node(name + "/batchnorm/sub", "Sub", [ins[1], name + "/batchnorm/mul_2"])
        b.node(name + "/batchnorm/add_1", "Add", [name + "/batchnorm/mul_1", name + "/batchnorm/sub"])
        b.node(name + "/cond/train_branch", "Neg", [name + "/cond/Switch_1:1"])      # hangs off port 1: must be dead
        b.node(name + "/cond/Merge", "Merge", [name + "/batchnorm/add_1", name + "/cond/train_branch"])
        return name + "/cond/Merge"

    def relu6(name, src):
        b.node(name + "/Relu6", "Relu6", [src])
        return name + "/Relu6"

    def pad(name, src, hw):
        p = correct_pad(hw)
        b.const(name + "/Pad/paddings", np.array([[0, 0], list(p), list(p), [0, 0]], np.int32))
        b.node(name + "/Pad", "Pad", [src, name + "/Pad/paddings"])
        return name + "/Pad"

    def out_hw(hw, stride):
        return (hw + stride - 1) // stride      # SAME and correct_pad + VALID agree on it

    def conv(name, src, k, cin, cout, stride, hw):
        b.const(name + "/kernel", (rs.randn(k, k, cin, cout) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32))
        padding = "SAME"
        if k == 3 and stride == 2 and style == "keras":
            src, padding = pad(name + "_pad", src, hw), "VALID"
        b.node(name + "/convolution", "Conv2D", [src, name + "/kernel"], strides=[1, stride, stride, 1], padding=padding, data_format="NHWC")
        return name + "/convolution"

    def depthwise(prefix, src, c, stride, hw):
        b.const(prefix + "depthwise/depthwise_kernel", (rs.randn(3, 3, c, 1) * np.sqrt(2.0 / 9)).astype(np.float32))
        padding = "SAME"
        if stride == 2 and style == "keras":
            src, padding = pad(prefix + "pad", src, hw), "VALID"
        b.node(prefix + "depthwise/depthwise", "DepthwiseConv2dNative", [src, prefix + "depthwise/depthwise_kernel"],
               strides=[1, stride, stride, 1], padding=padding, data_format="NHWC")
        return prefix + "depthwise/depthwise"

    c = make_divisible(32 * alpha, 8)
    widths = [c]
    x = relu6("Conv1_relu", batchnorm("bn_Conv1", conv("Conv1", "input_1", 3, 3, c, 2, size), c))
    hw = out_hw(size, 2)
    block_outputs = []
    for block_id, t, cout, stride in block_table(alpha, blocks):
        prefix = "block_%d_" % block_id if block_id else "expanded_conv_"
        y, mid = x, c
        if block_id:
            mid = t * c
            y = relu6(prefix + "expand_relu", batchnorm(prefix + "expand_BN", conv(prefix + "expand", y, 1, c, mid, 1, hw), mid))
        y = relu6(prefix + "depthwise_relu", batchnorm(prefix + "depthwise_BN", depthwise(prefix, y, mid, stride, hw), mid))
        hw = out_hw(hw, stride)
        y = batchnorm(prefix + "project_BN", conv(prefix + "project", y, 1, mid, cout, 1, hw), cout, damp=0.4)
        if cout == c and stride == 1:
            b.node(prefix + "add/add", "Add", [x, y])
            y = prefix + "add/add"
        block_outputs.append(y)
        x, c = y, cout
        widths += [mid, cout]
    last = last_width(alpha)
    x = relu6("out_relu", batchnorm("Conv_1_bn", conv("Conv_1", x, 1, c, last, 1, hw), last))
    widths.append(last)
    b.const(output + "/reduction_indices", np.array([1, 2], np.int32))
    b.node(output, "Mean", [x, output + "/reduction_indices"])
    return b.serialize(), {"widths": widths, "block_outputs": block_outputs, "features": last, "learning_phase": phase,
                           "final_hw": hw}
