"""Float64 reference of the fast (momentum) Griffin-Lim iteration (isp_tts_amd.griffinlim.FastGriffinLim), in two forms built
on tests/griffinlim_reference.py's stft, istft, project and initial:

    textbook             keeps the complex tprev = STFT(x_{n-1}) and takes the phase of STFT(x_n) - a tprev (librosa's and
                         torchaudio's loop), a = momentum / (1 + momentum), tprev = 0 before the first iteration
    waveform difference  the plain step applied to x_n - a x_{n-1}, x_{-1} = 0: what the kernel computes; equal by linearity of
                         the STFT

x_0 is the hashed start of `seed`, or `init`."""
import numpy as np

import griffinlim_reference as gr


def alpha(momentum: float) -> float:
    return momentum / (1.0 + momentum)


def _start(M, seed, init):
    return gr.initial(M, seed) if init is None else np.asarray(init, dtype=np.float64)


def textbook(M: np.ndarray, n_iter: int, momentum: float, seed: int = 0, init=None, keep=()):
    """n_iter fast iterations.  `keep`: iteration counts whose waveforms are returned as {count: waveform} instead of the last."""
    a, x = alpha(momentum), _start(M, seed, init)
    tprev = np.zeros(M.shape, dtype=complex)
    kept = {0: x} if 0 in keep else {}
    for i in range(1, n_iter + 1):
        rebuilt = gr.stft(x)
        x = gr.istft(gr.project(rebuilt - a * tprev, M))
        tprev = rebuilt
        if i in keep:
            kept[i] = x
    return kept if keep else x


def waveform_difference(M: np.ndarray, n_iter: int, momentum: float, seed: int = 0, init=None, keep=()):
    a, x = alpha(momentum), _start(M, seed, init)
    xprev = np.zeros_like(x)
    kept = {0: x} if 0 in keep else {}
    for i in range(1, n_iter + 1):
        x, xprev = gr.step(x - a * xprev, M), x
        if i in keep:
            kept[i] = x
    return kept if keep else x
