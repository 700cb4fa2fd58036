"""Adam(amsgrad=True) update — TEST INFRASTRUCTURE (see oracle/__init__).

Restates keras.optimizers.Adam(learning_rate, amsgrad=True) (pldepth/PLDepth.py:133) as TF
applies it per variable (ResourceApplyAdamWithAmsgrad functor; Keras defaults beta_1=0.9,
beta_2=0.999, epsilon=1e-7; local_step = iterations + 1; all in float32):
    alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
    m += (g - m) * (1 - b1);  v += (g*g - v) * (1 - b2);  vhat = max(vhat, v)
    p -= m * alpha / (sqrt(vhat) + eps)

``grad_scale`` is the data-parallel mean (1 / world) the HIP kernel folds into the update: the
gradient enters as ``g * float32(grad_scale)``, one float32 product, before anything else.
"""
import numpy as np


def adam_amsgrad_step(p, g, m, v, vhat, lr, step, beta1=0.9, beta2=0.999, eps=1e-7,
                      grad_scale=1.0):
    f = np.float32
    p, g, m, v, vhat = (np.asarray(a, np.float32).copy() for a in (p, g, m, v, vhat))
    g = g * f(grad_scale)
    b1p = f(np.power(f(beta1), f(step)))
    b2p = f(np.power(f(beta2), f(step)))
    alpha = f(f(lr) * np.sqrt(f(1) - b2p) / (f(1) - b1p))
    m += (g - m) * (f(1) - f(beta1))  # TF: T(1) - beta1 with float32 beta1
    v += (g * g - v) * (f(1) - f(beta2))
    vhat = np.maximum(vhat, v)
    p -= (m * alpha) / (np.sqrt(vhat) + f(eps))
    return p, m, v, vhat


def adam_amsgrad_step64(p, g, m, v, vhat, lr, step, beta1=0.9, beta2=0.999, eps=1e-7,
                        grad_scale=1.0):
    """The same update with every operation in float64. The inputs are what the float32 step
    sees: arrays and hyper-parameters are rounded to float32 first (beta1 = float32(0.9), not
    0.9), so the two differ by the float32 step's own rounding only. Returns (p, m, v, vhat)
    as float64 arrays."""
    d = np.float64

    def f(x):  # the float32 value the kernel is handed, held in float64
        return d(np.float32(x))

    p, g, m, v, vhat = (np.asarray(a, np.float32).astype(d) for a in (p, g, m, v, vhat))
    g = g * f(grad_scale)
    b1, b2 = f(beta1), f(beta2)
    t = d(step)
    alpha = f(lr) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    vhat = np.maximum(vhat, v)
    p = p - (m * alpha) / (np.sqrt(vhat) + f(eps))
    return p, m, v, vhat
