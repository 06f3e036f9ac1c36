"""CPU restatement of vd_lora_act_grad for the tests (a helper module, not a test file; no GPU needed): the adapter gradient of a 1x1 layer
y_b = W x_b, W = W0 + s B A, straight from its activations in float64, with the derived error bounds of the f32 kernel.

    dA[q][l] = s sum_{b,p} (sum_m Bm[m][q] dy[b][m][p]) x[b][l][p]          dB[m][q] = s sum_{b,p} dy[b][m][p] (sum_l A[q][l] x[b][l][p])

dy: [B, M, N], x: [B, L, N], A: [r, L], Bm: [M, r]."""
import torch

U = 2.0 ** -24          # unit round-off of f32


def grads(dy, x, A, Bm, s):
    """(dA [r, L], dB [M, r]) in float64."""
    dy, x, A, Bm = dy.double(), x.double(), A.double(), Bm.double()
    T = torch.einsum("mq,bmp->bqp", Bm, dy)
    Z = torch.einsum("ql,blp->bqp", A, x)
    return s * torch.einsum("bqp,blp->ql", T, x), s * torch.einsum("bmp,bqp->mq", dy, Z)


def weight_grad(dy, x):
    """G = sum_b dy_b x_b^T [M, L] in float64: the ordinary weight gradient the closed forms of lora_ref.grads start from."""
    return torch.einsum("bmp,blp->ml", dy.double(), x.double())


def bounds(dy, x, A, Bm, s):
    """(bound of dA, bound of dB).  An element of dB is a sum of L * B * N triple products dy * A * x evaluated in two levels (the inner sum over
    l has L addends, the outer over (b, p) has B * N): every product is rounded twice, every addition once, plus the partial-sum additions of
    the reduce and the product with s -- at most L + B N + 4 roundings touch any term, and with a factor 2 to spare
        |err| <= 2 (L + B N + 4) u |s| sum |dy| |A| |x|
    for ANY order of the two sums.  dA likewise with M for L and |Bm| for |A|."""
    dy, x, A, Bm = dy.double().abs(), x.double().abs(), A.double().abs(), Bm.double().abs()
    Bn, M, N = dy.shape
    L = x.shape[1]
    mA, mB = grads(dy, x, A, Bm, abs(s))
    return 2 * (M + Bn * N + 4) * U * mA, 2 * (L + Bn * N + 4) * U * mB
