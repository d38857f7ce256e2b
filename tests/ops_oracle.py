"""float64 oracles, error bounds and input builders for the kernels bound in csrc/binding/ops.cpp
(sgd.hip, xent.hip, flat_ops.hip, augment.hip), used by tests/test_ops_edges_gpu.py and checked on
the CPU by tests/test_ops_oracles_cpu.py.

Every oracle is the operation written out from its formula in float64 on the same input values.
Nothing here imports the package: the constants of the CIFAR transform are written out. Builders
draw from a CPU generator and move the result to the device they are given, so the CPU check and
the GPU test see the same values.
"""
import torch

F32 = torch.float32
U = 2.0 ** -24  # one fp32 rounding, relative

# ToTensor + Normalize of the CIFAR-10 transform (mean and std of the 0..255 pixel values)
CIFAR_MEAN_255 = (125.3, 123.0, 113.9)
CIFAR_STD_255 = (63.0, 62.1, 66.7)
PAD = 4


def _d(t):
    return t.detach().double()


def f32(v):
    """a Python float rounded to fp32, as a kernel receives it"""
    return float(torch.tensor(float(v), dtype=F32))


def bits_of(x):
    """the bit pattern of an fp32 / bf16 tensor as non-negative int64"""
    if x.dtype == F32:
        return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert x.dtype == torch.bfloat16
    return x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def f32_from_bits(bits, device):
    """fp32 tensor with the given 32-bit patterns (ints in [0, 2^32))"""
    b = torch.as_tensor(bits, dtype=torch.int64)
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(F32).to(device)


def bf16_from_bits(bits, device):
    """bf16 tensor with the given 16-bit patterns (ints in [0, 2^16))"""
    b = torch.as_tensor(bits, dtype=torch.int64)
    b = torch.where(b >= 2 ** 15, b - 2 ** 16, b).to(torch.int16)
    return b.view(torch.bfloat16).to(device)


# ------------------------------------------------------------------ SGD
# (lr, momentum, weight_decay, dampening, scale, first)
SGD_CONFIGS = [
    (0.1, 0.9, 1e-4, 0.0, 1.0, False),
    (0.05, 0.8, 5e-4, 0.25, 0.5, False),
    (0.1, 0.9, 0.0, 0.1, 3.0, False),
    (0.1, 0.9, 1e-4, 0.0, 1.0, True),
    (0.1, 0.0, 1e-4, 0.0, 1.0, False),
]


def _sgd_hyper(lr, mom, wd, damp, scale):
    """the hyperparameters as the kernel gets them: rounded to fp32, 1 - damp formed in fp32"""
    omd = float(torch.tensor(1.0, dtype=F32) - torch.tensor(float(damp), dtype=F32))
    return f32(lr), f32(mom), f32(wd), omd, f32(scale)


def sgd_oracle(p, g, m, lr, mom, wd, damp, scale, first):
    """d = g scale + wd p; buf = d if first else mom m + (1 - damp) d; p' = p - lr buf. With mom == 0
    buf = d and m comes back unchanged; with first m is not read. Returns (p', m') in float64."""
    lr, mom, wd, omd, scale = _sgd_hyper(lr, mom, wd, damp, scale)
    p, g = _d(p), _d(g)
    d = g * scale + wd * p
    if mom == 0:
        return p - lr * d, _d(m)
    buf = d if first else mom * _d(m) + omd * d
    return p - lr * buf, buf


def sgd_bounds(p, g, m, lr, mom, wd, damp, scale, first):
    """(bound on |p' - p'64|, bound on |m' - m'64|) per element. T_d = |g scale| + wd |p| is the sum of
    the magnitudes that make d, T_m = mom |m| + |1 - damp| T_d (T_d if first or mom == 0) of those that
    make the buffer. m' is at most 4 roundings of terms of T_m (g scale, the fma, m mom, the fma);
    p' adds the product by lr and the final fma: 6 roundings of |p| + lr T_m."""
    lr, mom, wd, omd, scale = _sgd_hyper(lr, mom, wd, damp, scale)
    p, g = _d(p).abs(), _d(g).abs()
    t_d = g * abs(scale) + wd * p
    t_m = t_d if (first or mom == 0) else mom * _d(m).abs() + abs(omd) * t_d
    return 6 * U * (p + lr * t_m), 4 * U * t_m


def sgd_inputs(n, device, seed=0):
    """p, g, m of n elements, random sign, magnitudes log-uniform in [1e-3, 1e3]"""
    g_ = torch.Generator(device="cpu").manual_seed(1000 + seed)

    def one():
        mag = torch.pow(10.0, torch.rand(n, generator=g_, dtype=torch.float64) * 6 - 3)
        sign = torch.randint(0, 2, (n,), generator=g_, dtype=torch.float64) * 2 - 1
        return (mag * sign).float().to(device)

    return one(), one(), one()


# ------------------------------------------------------------------ classifier head
def head_oracle(feat, W, bias, labels, gscale=1.0):
    """logits = feat W^T + bias; loss = mean_b (log sum_j exp logits[b, j] - logits[b, y_b]);
    dlogits = (softmax - onehot) gscale / B; dW = dlogits^T feat; db = sum_b dlogits; dfeat = dlogits W.
    The logits are summed class by class with one expression, so bit-equal rows of W with equal biases
    give bit-equal logits. Returns (logits, loss, dlogits, dW, db, dfeat) in float64."""
    feat, W, bias = _d(feat), _d(W), _d(bias)
    B, C = feat.shape[0], W.shape[0]
    logits = torch.stack([(feat * W[j]).sum(1) + bias[j] for j in range(C)], 1)
    loss, dl = xent_oracle(logits, labels, gscale)
    return logits, loss, dl, dl.t() @ feat, dl.sum(0), dl @ W


def xent_oracle(logits, labels, gscale=1.0):
    """mean softmax cross-entropy of [B, C] logits and dlogits = (softmax - onehot) gscale / B, float64"""
    x = _d(logits)
    B = x.shape[0]
    mx = x.max(1, keepdim=True).values
    lse = (x - mx).exp().sum(1).log() + mx[:, 0]
    rows = torch.arange(B, device=x.device)
    loss = (lse - x[rows, labels]).mean()
    dl = (x - lse[:, None]).exp()
    dl[rows, labels] -= 1.0
    return loss, dl * (f32(gscale) / B)


HEAD_NAMES = ("logits", "loss", "dlogits", "dW", "db", "dfeat")


def head_bounds(ref, gscale, peaked=None):
    """per output of head_oracle the bound on |got - ref| (a tensor or a number), by name. Against
    float64 with the tolerances tests/test_ops_gpu.py applies to the same outputs: logits rtol = atol =
    1e-5; dlogits, dW, db, dfeat rtol 1e-4, atol 1e-6 gscale (the gradients are linear in gscale); the
    loss, a difference of two logit-sized numbers, 1e-5 (1 + max |logit|).

    peaked = (feat, W, bias) for the cases with scaled features. There fp32 logits cannot be better
    than e_b = n 2^-24 max_j (sum_k |feat[b, k] W[j, k]| + |bias[j]|) in absolute terms, n = 4 ceil(K / 256)
    + 8 the roundings of the longest chain (per lane 4 products added per float4 and trip, 6 cross-lane
    additions, the bias, a product), and rtol |logit| of a logit that is small after cancellation is
    far below it. Logits shifted by at most e give softmax values within a factor exp(+-2 e) of p,
    and the same holds for 1 - p (a sum of the others), so p moves by at most
    t = min(p, 1 - p) (exp(2 e_b) - 1): nothing where the softmax is saturated, e / 2 at a tie.
    dlogits[b, j] moves by s = (gscale / B) t, and with it db[j] by sum_b s, dW[j, k] by
    sum_b s |feat[b, k]| and dfeat[b, k] by sum_j s |W[j, k]|. dW's own sum grows with the features
    too, beyond an atol meant for unit ones: (B + 8) 2^-24 sum_b |dlogits[b, j] feat[b, k]| (B additions, a
    product, at most 7 roundings inside a dlogits value). These terms (and e_b for the logits) are
    added to the tolerances above; the loss bound already scales with the logits."""
    logits = ref[0]
    B = logits.shape[0]
    grad = (1e-4, 1e-6 * gscale)
    tol = dict(logits=(1e-5, 1e-5), loss=(0.0, 1e-5 * (1 + float(logits.abs().max()))), dlogits=grad, dW=grad,
               db=grad, dfeat=grad)
    out = {n: tol[n][1] + tol[n][0] * r.abs() for n, r in zip(HEAD_NAMES, ref)}
    if peaked is not None:
        feat, W, bias = (_d(t).abs() for t in peaked)
        n = 4 * -(-feat.shape[1] // 256) + 8
        e = n * U * (feat @ W.t() + bias).max(1).values
        p = torch.softmax(logits, 1)
        s = f32(gscale) / B * torch.minimum(p, 1 - p) * torch.expm1(2 * e)[:, None]  # [B, C]
        out["logits"] = out["logits"] + e[:, None]
        out["dlogits"] = out["dlogits"] + s
        out["db"] = out["db"] + s.sum(0)
        out["dW"] = out["dW"] + s.t() @ feat + (B + 8) * U * (ref[2].abs().t() @ feat)
        out["dfeat"] = out["dfeat"] + s @ W
    return out


def lowest_argmax(x):
    """per row the lowest index that holds the row maximum"""
    C = x.shape[1]
    idx = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def head_inputs(B, K, C, device, seed=0):
    """feat ~ N(0, 1) [B, K], W ~ 0.05 N(0, 1) [C, K], bias ~ N(0, 1) [C], labels uniform in [0, C)"""
    g_ = torch.Generator(device="cpu").manual_seed(7000 + seed + B * 100003 + K * 131 + C)
    feat = torch.randn(B, K, generator=g_)
    W = torch.randn(C, K, generator=g_) * 0.05
    bias = torch.randn(C, generator=g_)
    y = torch.randint(0, C, (B,), generator=g_)
    return feat.to(device), W.to(device), bias.to(device), y.to(device)


def peak_scale(feat, W, bias, target):
    """the power of two s for which max |logit| of (s feat, W, bias) is nearest to target (in log2);
    scaling by it is exact"""
    lg = head_oracle(feat, W, torch.zeros_like(bias), torch.zeros(feat.shape[0], dtype=torch.long,
                                                                  device=feat.device))[0]
    return 2.0 ** round(float(torch.log2(target / lg.abs().max())))


TIE_PAIR = (3, 7)


def head_tie_inputs(B, K, C, device, variant):
    """'flat': W = 0 and every bias 0.5, so every logit is 0.5 and every class ties.
    'pair': rows TIE_PAIR of W bit-equal and their biases both 50, every other bias in [-1, 1]: the two
    logits of a sample are bit-equal (same products, same order) and, at |feat W^T| well below 49,
    the row's maximum. The lowest index of the maximum is 0 ('flat') or TIE_PAIR[0] ('pair')."""
    feat, W, bias, y = head_inputs(B, K, C, device, seed=5)
    if variant == "flat":
        return feat, torch.zeros_like(W), torch.full_like(bias, 0.5), y
    assert variant == "pair" and C > TIE_PAIR[1]
    W, bias = W.clone(), bias.clamp(-1, 1)
    W[TIE_PAIR[1]] = W[TIE_PAIR[0]]
    bias[TIE_PAIR[0]] = bias[TIE_PAIR[1]] = 50.0
    return feat, W, bias, y


def xent_inputs(B, C, device, seed=0):
    """logits ~ 3 N(0, 1) [B, C] and labels uniform in [0, C)"""
    g_ = torch.Generator(device="cpu").manual_seed(9000 + seed + B * 131 + C)
    return (torch.randn(B, C, generator=g_) * 3).to(device), torch.randint(0, C, (B,), generator=g_).to(device)


# ------------------------------------------------------------------ flat combines and casts
def rows_mean_oracle(src, rows):
    """(mean over the rows of src [rows * n] in float64, the bound rows 2^-24 sum_r |src_r| / rows:
    rows - 1 additions and one division, each one rounding of at most the sum of magnitudes)"""
    s = _d(src).view(rows, -1)
    return s.sum(0) / rows, rows * U * s.abs().sum(0) / rows


def bf16_rne_bits(x):
    """the bf16 bit pattern (int64 in [0, 2^16)) of fp32 x rounded to nearest, ties to even, in integer
    arithmetic on the fp32 bits: add 0x7fff plus the kept bit, drop 16 bits (a carry out of the
    mantissa runs into the exponent, up to Inf). A NaN keeps its top bits and gets a quiet bit."""
    u = bits_of(x)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(nan, (u >> 16) | 0x40, r)


def bf16_bits_isnan(b):
    return (b & 0x7FFF) > 0x7F80


# fp32 bit patterns outside the normal range, with the bf16 pattern each must become (None: any NaN)
CAST_SPECIALS = [
    (0x00000000, 0x0000), (0x80000000, 0x8000),                          # +-0
    (0x00000001, 0x0000), (0x80000001, 0x8000),                          # the smallest subnormals -> +-0
    (0x007FFFFF, 0x0080), (0x807FFFFF, 0x8080),                          # the largest -> the smallest normal
    (0x00008000, 0x0000), (0x00018000, 0x0002), (0x00004000, 0x0000),    # subnormal ties and below
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80),                          # the largest finite float -> Inf
    (0x7F7F7FFF, 0x7F7F), (0xFF7F7FFF, 0xFF7F),                          # the largest that stays finite
    (0x7F7F8000, 0x7F80), (0x7F7E8000, 0x7F7E),                          # the ties around it
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),                          # +-Inf
    (0x7FC00000, None), (0xFFC00001, None), (0x7F800001, None), (0x7FFFFFFF, None),  # NaNs
]


def cast_edge_inputs(n, device, seed=0):
    """fp32 [n]: CAST_SPECIALS, then for every hi16 with a finite exponent (both parities of the kept
    bit, subnormals included) the exact tie hi16 << 16 | 0x8000 and its neighbours one ulp below and
    above, then random values of magnitudes 1e-3 .. 1e3. Returns (x, number of built elements)."""
    hi = torch.arange(0x10000, dtype=torch.int64)
    hi = hi[(hi & 0x7F80) != 0x7F80]
    tie = (hi << 16) | 0x8000
    built = torch.cat([torch.tensor([b for b, _ in CAST_SPECIALS], dtype=torch.int64), tie, tie - 1, tie + 1])
    assert built.numel() <= n
    head = f32_from_bits(built, "cpu")
    g_ = torch.Generator(device="cpu").manual_seed(300 + seed)
    k = n - built.numel()
    rnd = torch.randn(k, generator=g_) * torch.pow(10.0, torch.rand(k, generator=g_) * 6 - 3)
    return torch.cat([head, rnd.float()]).to(device), built.numel()


def backcast_inputs(n, device, seed=0):
    """bf16 [n] as bit patterns (int64): all 2^16 patterns, NaNs included, then random ones"""
    g_ = torch.Generator(device="cpu").manual_seed(400 + seed)
    assert n >= 0x10000
    bits = torch.cat([torch.arange(0x10000, dtype=torch.int64),
                      torch.randint(0, 0x10000, (n - 0x10000,), generator=g_)])
    return bf16_from_bits(bits, device), bits.to(device)


# ------------------------------------------------------------------ augment
AUG_N = 18


def augment_dataset(device):
    """data[n, y, x, c] = (7 n + 3 (32 y + x) + c) % 251, uint8 [18, 32, 32, 3]: a pixel differs from
    its four neighbours, from its mirror image and from its transpose (the checks are in the CPU
    test), so a transposition, a flip before the crop or an off-by-one changes values. params: every
    (dy, dx) in {0, 4, 8}^2 x flip in {0, 1}, int32 [18, 3], image n gets combination n."""
    n = torch.arange(AUG_N)[:, None, None, None]
    y = torch.arange(32)[None, :, None, None]
    x = torch.arange(32)[None, None, :, None]
    c = torch.arange(3)[None, None, None, :]
    data = ((7 * n + 3 * (32 * y + x) + c) % 251).to(torch.uint8)
    params = torch.tensor([(dy, dx, fl) for dy in (0, 4, 8) for dx in (0, 4, 8) for fl in (0, 1)], dtype=torch.int32)
    return data.to(device), params.to(device)


AUG_IDX = [list(range(AUG_N)), [17, 0, 0, 5], [3]]


def augment_oracle(data_u8, idx, params, nhwc, cstride=3):
    """RandomCrop(32, padding 4) + RandomHorizontalFlip + ToTensor + Normalize from their definitions:
    zero-pad the uint8 image by 4, take the 32 x 32 window at (dy, dx), mirror the window if fl,
    then x / 255, minus the mean, over the std per channel (float64). NHWC with cstride 4 gets a
    channel 3 of zeros; otherwise NCHW or NHWC with 3 channels."""
    mean = torch.tensor(CIFAR_MEAN_255, dtype=torch.float64, device=data_u8.device) / 255
    std = torch.tensor(CIFAR_STD_255, dtype=torch.float64, device=data_u8.device) / 255
    out = []
    for s in idx.tolist():
        dy, dx, fl = (int(v) for v in params[s].tolist())
        padded = torch.zeros(32 + 2 * PAD, 32 + 2 * PAD, 3, dtype=torch.uint8, device=data_u8.device)
        padded[PAD:PAD + 32, PAD:PAD + 32] = data_u8[s]
        win = padded[dy:dy + 32, dx:dx + 32]
        if fl:
            win = win.flip(1)
        out.append((win.double() / 255 - mean) / std)
    out = torch.stack(out)  # [B, 32, 32, 3]
    if not nhwc:
        return out.permute(0, 3, 1, 2).contiguous()
    if cstride == 4:
        out = torch.cat([out, torch.zeros_like(out[..., :1])], -1)
    return out
