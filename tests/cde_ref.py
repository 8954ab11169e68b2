"""float64 CPU restatement of the Neural-CDE motion latent (models/mocogan_cde.py) for the CDE tests.

* the path: torchcde's hermite_cubic_coefficients_with_backward_differences on the knots t = 0, 1, ..., T-1 of the
  two channels [linspace(0, 1, T) (fp32), x]: on [k, k+1] the endpoint slopes are d_{k-1} and d_k (d_k = x_{k+1} - x_k,
  d_{-1} := d_0); derivative b + (2c + 3d s) s with torchcde's interval choice (bucketize - 1, clamped);
* the vector field tanh(W2 relu(W1 z + b1) + b2).view(16, 2) @ dX/dt and the pre-net f([0, x_0]);
* replay(): the kernel's arithmetic in float64 on a GIVEN accepted schedule (autograd-transparent), so outputs, states
  and gradients can be compared exactly with the kernels'; with fp32 parameters the same arithmetic in torch's fp32, which
  measures the rounding error of the restatement itself on that schedule;
* solve(): a full float64 dopri5 solve with oracle.ode_ref's controller (whole-batch RMS norm).
"""
import numpy as np
import torch

from oracle import ode_ref

A = ((), (1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9),
     (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
     (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
ALPHA = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
CMID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
        187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


def time_slopes(T):
    tt = torch.linspace(0, 1, T).float()
    return (tt[1:] - tt[:-1]).double()


def slopes(v):
    """v [..., T] knot values -> d [..., T-1] (t_diff = 1)."""
    return v[..., 1:] - v[..., :-1]


def hermite_coeffs(d):
    """per-interval (b, 2c, 3d) of the derivative b + (2c + 3d s) s from the slopes d [..., T-1]."""
    b = torch.cat([d[..., :1], d[..., :-1]], dim=-1)
    c2 = 2 * (3 * (d - b) - d + b)
    d3 = (d - b) - c2
    return b, c2, d3


def interval(t, T):
    k = int(np.ceil(t)) - 1
    k = min(max(k, 0), T - 2)
    return k, t - k


def spline_value(x0, coeffs, t, T):
    """X(t) for one channel: x0 [..., T] knots."""
    b, c2, d3 = coeffs
    k, s = interval(t, T)
    return x0[..., k] + (b[..., k] + (c2[..., k] / 2 + d3[..., k] / 3 * s) * s) * s


def spline_deriv(coeffs, t, T):
    b, c2, d3 = coeffs
    k, s = interval(t, T)
    return b[..., k] + (c2[..., k] + d3[..., k] * s) * s


def params_of(gen, dtype=torch.float64):
    """the 8 live tensors in gode_cde_params order (Wa, ba, Wb, bb, W1, b1, W2, b2) as leaf copies"""
    fn = gen.ode_fn
    ps = [gen.f[0].weight, gen.f[0].bias, gen.f[2].weight, gen.f[2].bias, fn.linear1.weight, fn.linear1.bias,
          fn.linear2.weight, fn.linear2.bias]
    return [p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in ps]


def prenet(P, x0):
    """f([0, x_0]): x0 [N] -> [N, 16]"""
    Wa, ba, Wb, bb = P[:4]
    inp = torch.stack([torch.zeros_like(x0), x0], dim=-1)
    h = torch.nn.functional.leaky_relu(inp @ Wa.t() + ba, 0.2)
    return torch.nn.functional.leaky_relu(h @ Wb.t() + bb, 0.2)


class Field:
    """dz/dt(t, z) = tanh(W2 relu(W1 z + b1) + b2).view(N, 16, 2) @ dX/dt(t), z [N, 16]."""

    def __init__(self, P, x, T, round_time=True):
        self.P, self.T, self.round = P, T, round_time
        self.margin = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)   # min |W1 z + b1| seen
        xd = x.to(P[0].dtype)                          # float64 leaves: the reference; fp32: its own rounding error
        self.cx = hermite_coeffs(slopes(xd))
        self.ct = hermite_coeffs(time_slopes(T).to(P[0].dtype))

    def __call__(self, t, z):
        t = float(t)
        if self.round:
            t = float(np.float32(t))
        D0 = spline_deriv(self.ct, t, self.T)
        D1 = spline_deriv(self.cx, t, self.T)
        W1, b1, W2, b2 = self.P[4:]
        u1 = z @ W1.t() + b1
        self.margin = torch.minimum(self.margin, u1.detach().abs().min(dim=1).values.to(self.margin.dtype))
        F = torch.tanh(torch.relu(u1) @ W2.t() + b2).view(z.shape[0], 16, 2)
        return F[..., 0] * D0 + F[..., 1] * D1[:, None]


def interp_weights(x):
    x2, x3, x4 = x * x, x ** 3, x ** 4
    return (-8 * x4 + 14 * x3 - 5 * x2, 16 * x4 - 32 * x3 + 16 * x2, -2 * x4 + 5 * x3 - 4 * x2 + x, 2 * x4 - 3 * x3 + x2)


def replay(P, x, T, sched_t, sched_h, margin=None, round_abscissa=True):
    """The discrete forward on a given accepted schedule: -> (outputs [N, T, 16], states [N, S+1, 16], z0).
    round_abscissa: the dense output's abscissa from the fp32-rounded times, as the kernel and torchdiffeq on an fp32
    clock take it; False: from the float64 times, as solve() below (oracle.ode_ref._interp_eval on a float64 clock).
    margin (a dict): margin["relu"] = per trajectory, the smallest |W1 z + b1| of any stage -- where it is within
    rounding of 0, an fp32 and a float64 evaluation may take different ReLU branches (a kink of the exact gradient)."""
    f = Field(P, x, T)
    z0 = prenet(P, x[:, 0].to(P[0].dtype))
    y = z0
    outs = [z0]
    states = [z0]
    jo = 1
    for t0, h in zip(sched_t, sched_h):
        t0, h = float(t0), float(h)
        t1 = t0 + h
        ks = []
        for st in range(6):
            zi = y
            for coef, k in zip(A[st], ks):
                zi = zi + h * coef * k
            ks.append(f(t0 + ALPHA[st] * h, zi))
        y1 = y
        for coef, k in zip(B, ks):
            if coef:
                y1 = y1 + h * coef * k
        if jo < T and jo <= t1:
            k7 = f(t1, y1)
            ym = y
            for coef, k in zip(CMID, ks + [k7]):
                if coef:
                    ym = ym + h * coef * k
            while jo < T and jo <= t1:
                if round_abscissa:
                    xa = (float(np.float32(jo)) - float(np.float32(t0))) / (float(np.float32(t1)) - float(np.float32(t0)))
                else:
                    xa = (jo - t0) / (t1 - t0)
                wS, wM, w1, w7 = interp_weights(xa)
                outs.append(y + wS * (y1 - y) + wM * (ym - y) + h * (w1 * ks[0] + w7 * k7))
                jo += 1
        y = y1
        states.append(y)
    assert jo == T, "the schedule does not reach the last output time"
    if margin is not None:
        margin["relu"] = f.margin
    return torch.stack(outs, 1), torch.stack(states, 1), z0


def solve(P, x, T, rtol=1e-4, atol=1e-6, sched=None):
    """float64 dopri5 of oracle.ode_ref with the whole-batch RMS norm -> (outputs [N, T, 16], accepted, trials); sched (a
    list) receives the accepted steps as (t0, h) floats, in order (the solve stops with the step that reaches T - 1).  The
    stage times reach the field rounded to fp32, as oracle.ode_ref.dopri5_solve and torchdiffeq pass them to an fp32
    field (the step counts are sensitive to it: 54 / 82 instead of 56 / 90 accepted / trial steps at N = 32, seed 7)."""
    f = Field(P, x, T)
    z0 = prenet(P, x[:, 0].double())
    calls = {"acc": 0, "trials": 0, "sched": sched}
    out = _dopri5_counted(f, z0, torch.arange(T, dtype=torch.float64), rtol, atol, calls)
    return out.transpose(0, 1), calls["acc"], calls["trials"]


def _dopri5_counted(f, y0, t, rtol, atol, calls):
    """oracle.ode_ref.dopri5_solve's loop on its own controller pieces (_initial_step, tableau, _interp_fit /
    _interp_eval, factor clipping), with the accepted and trial steps counted."""
    R = ode_ref
    tt = t.to(torch.float64)
    y = y0
    t0 = tt[0]
    f0 = f(t0, y)
    dt = R._initial_step(f, tt[0], y0, 4, rtol, atol, R._rms, f0).to(torch.float64)
    interp, seg0, seg1 = (y,) * 5, t0, t0
    out = [y0]
    for j in range(1, len(tt)):
        target = tt[j]
        while target > seg1:
            ks = [f0]
            for alpha, beta in zip(R._DP_ALPHA, R._DP_BETA):
                yi = y + sum(k * (b * dt) for k, b in zip(ks, beta))
                ks.append(f(t0 + alpha * dt, yi))
            y1, f1 = yi, ks[-1]
            err = sum(k * (c * dt) for k, c in zip(ks, R._DP_CERR))
            ratio = R._rms(err / (atol + rtol * torch.max(y.abs(), y1.abs())))
            calls["trials"] += 1
            if bool(ratio <= 1):
                calls["acc"] += 1
                if calls.get("sched") is not None:
                    calls["sched"].append((float(t0), float(dt)))
                y_mid = y + sum(k * (c * dt) for k, c in zip(ks, R._DP_CMID))
                interp = R._interp_fit(y, y1, y_mid, f0, f1, dt)
                seg0, seg1 = t0, t0 + dt
                t0, y, f0 = t0 + dt, y1, f1
            if ratio == 0:
                dt = dt * 10.0
            else:
                dt = dt * torch.clamp(0.9 * ratio ** (-0.2), min=1.0 if ratio < 1 else 0.2, max=10.0)
        out.append(R._interp_eval(interp, seg0, seg1, target))
    return torch.stack(out)


def continuous_adjoint(P, x, T, gout, rtol=1e-4, atol=1e-6):
    """torchdiffeq's odeint_adjoint (oracle.ode_ref, continuous adjoint) of sum(out * gout) w.r.t. the 8 tensors."""
    Pc = [p.detach().clone().requires_grad_(True) for p in P]
    f = Field(Pc, x, T)

    class Fn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(p) for p in Pc[4:]])

        def forward(self, t, z):
            f.P = list(Pc[:4]) + list(self.ps)
            return f(t, z)

    m = Fn()
    z0 = prenet(Pc, x[:, 0].double())
    out = ode_ref.odeint_adjoint(m, z0, torch.arange(T, dtype=torch.float64), rtol=rtol, atol=atol, method="dopri5")
    loss = (out.transpose(0, 1) * gout).sum()
    gs = torch.autograd.grad(loss, list(Pc[:4]) + list(m.ps))
    return gs
