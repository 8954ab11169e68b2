"""Float64 restatement of the GRU motion latent (models/mocogan.py:217-229) and of its backpropagation through time --
what csrc/gru_valu.hip computes, written out step by step in NumPy so that the kernels can be checked against it and it
can be checked against torch.autograd on an nn.GRUCell chain (tests/test_host_gru.py).

Shapes: noise [T+1, N, 16] = h_0, e_0 .. e_{T-1};  hs [N, T+1, 16] = h_0 .. h_T;  latent row n*T + t = h_{t+1};
weights in torch's GRUCell layout (weight_ih, weight_hh [48, 16], bias_ih, bias_hh [48], gate order r, z, n).
"""
import numpy as np

NPARAM = 1632


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _gates(Wih, Whh, bih, bhh, e, h):
    gi = e @ Wih.T + bih
    gh = h @ Whh.T + bhh
    r = _sigmoid(gi[:, :16] + gh[:, :16])
    z = _sigmoid(gi[:, 16:32] + gh[:, 16:32])
    hn = gh[:, 32:]
    n = np.tanh(gi[:, 32:] + r * hn)
    return r, z, n, hn


def forward(Wih, Whh, bih, bhh, noise):
    """-> hs [N, T+1, 16] (float64)."""
    Wih, Whh, bih, bhh, noise = (np.asarray(a, np.float64) for a in (Wih, Whh, bih, bhh, noise))
    T = noise.shape[0] - 1
    h = noise[0]
    hs = [h]
    for t in range(T):
        r, z, n, _ = _gates(Wih, Whh, bih, bhh, noise[t + 1], h)
        h = (1.0 - z) * n + z * h
        hs.append(h)
    return np.stack(hs, axis=1)


def latent_rows(hs):
    """[N, T+1, 16] -> the latent rows [N*T, 16] (row n*T + t = h_{t+1})."""
    return hs[:, 1:].reshape(-1, hs.shape[-1])


def backward(Wih, Whh, bih, bhh, noise, hs, g_rows):
    """g_rows [N, T, 16]: dL/dh_{t+1} from the latent rows -> the 1632 parameter gradients in the kernel's order
    (weight_ih, weight_hh, bias_ih, bias_hh), float64."""
    Wih, Whh, bih, bhh, noise, hs, g_rows = (np.asarray(a, np.float64) for a in (Wih, Whh, bih, bhh, noise, hs, g_rows))
    T = noise.shape[0] - 1
    gWih, gWhh = np.zeros_like(Wih), np.zeros_like(Whh)
    gbih, gbhh = np.zeros_like(bih), np.zeros_like(bhh)
    carry = np.zeros_like(hs[:, 0])
    for t in range(T - 1, -1, -1):
        e, h = noise[t + 1], hs[:, t]
        r, z, n, hn = _gates(Wih, Whh, bih, bhh, e, h)
        gh = carry + g_rows[:, t]
        dn = gh * (1.0 - z) * (1.0 - n * n)
        dz = gh * (h - n) * z * (1.0 - z)
        dr = dn * hn * r * (1.0 - r)
        dgi = np.concatenate([dr, dz, dn], axis=1)          # d/d(W_i e + b_i)
        dgh = np.concatenate([dr, dz, dn * r], axis=1)      # d/d(W_h h + b_h)
        gWih += dgi.T @ e
        gWhh += dgh.T @ h
        gbih += dgi.sum(0)
        gbhh += dgh.sum(0)
        carry = gh * z + dgh @ Whh
    return np.concatenate([gWih.ravel(), gWhh.ravel(), gbih, gbhh])


def split(grads):
    """1632 floats -> (weight_ih [48,16], weight_hh [48,16], bias_ih [48], bias_hh [48])."""
    return grads[:768].reshape(48, 16), grads[768:1536].reshape(48, 16), grads[1536:1584], grads[1584:1632]
