"""
Self-play draws on the device (``config.device_draws``; csrc/mzx_draws.h holds the definition): Dirichlet noise of the
roots, tie-break tape and action choice as a pure function of (seed, stream, counter) over Philox4x32-10 -- thin wrappers
of ``mzx_selfplay_draws`` / ``mzx_selfplay_select_device``.  Not numpy's draws, hence opt-in; no host stream is touched.
"""
import ctypes

import numpy
import torch

from . import _lib

MAX_ACTIONS = 4096


def _dev(backend, a, dtype):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(device=backend.device, dtype=dtype).contiguous()
    return torch.as_tensor(numpy.ascontiguousarray(a)).to(dtype).to(backend.device)


def _header(backend, seed, counter, num_games, action_space_size, streams, first_stream, keep):
    d = _lib.Draws()
    d.seed, d.counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    t_streams = _dev(backend, streams, torch.int32)
    if t_streams is not None and tuple(t_streams.shape) != (num_games,):
        raise ValueError("streams: one entry per game")
    keep.append(t_streams)
    d.d_streams = backend.ptr(t_streams)
    d.first_stream, d.num_games, d.action_space_size = int(first_stream), int(num_games), int(action_space_size)
    return d


def root_draws(backend, seed, counter, num_games, action_space_size, tape_words, alpha=0.0, legal=None, n=None,
               streams=None, first_stream=0, noise=True):
    """
    Noise [B][A] float64 (None with ``noise=False``) and tape [B][tape_words] int32 (the uint32 words' bits) of B roots,
    as device tensors.  ``legal`` [B][A] padded with -1, or ``n`` [B] children per root.  One launch, no synchronisation.
    """
    keep = []
    d = _header(backend, seed, counter, num_games, action_space_size, streams, first_stream, keep)
    t_legal, t_n = _dev(backend, legal, torch.int32), _dev(backend, n, torch.int32)
    if t_legal is not None and tuple(t_legal.shape) != (num_games, action_space_size):
        raise ValueError("legal: [num_games][action_space_size]")
    if t_n is not None and tuple(t_n.shape) != (num_games,):
        raise ValueError("n: one entry per game")
    t_noise = backend.empty((num_games, action_space_size), torch.float64) if noise else None
    t_tape = backend.empty((num_games, max(int(tape_words), 0)), torch.int32)
    d.tape_words, d.dirichlet_alpha = int(tape_words), float(alpha)
    d.d_legal_actions, d.d_n, d.d_noise, d.d_tape = (backend.ptr(t_legal), backend.ptr(t_n), backend.ptr(t_noise),
                                                     backend.ptr(t_tape))
    backend.lib.check(backend.lib.mzx_selfplay_draws(ctypes.byref(d), backend.stream()))
    return t_noise, t_tape


def power_table(temperatures, stride):
    """numpy's own ``int32 ** (1 / T)`` over 0 .. stride - 1 for the distinct finite non-zero temperatures (the expression of
    SelfPlay.select_action): (table [k][stride] or None, temperatures [k])."""
    temps = numpy.atleast_1d(numpy.asarray(temperatures, dtype=numpy.float64))
    key = numpy.unique(temps[(temps != 0) & ~numpy.isinf(temps)])
    if not key.size:
        return None, key
    return numpy.ascontiguousarray(numpy.stack([numpy.arange(stride, dtype="int32") ** (1 / float(t)) for t in key])), key


def select(backend, seed, counter, legal, visits, temperature, table=None, table_temperatures=None, streams=None,
           first_stream=0, uniforms=None):
    """The action [B] int64 (device tensor) of every game: ``mzx_selfplay_select_device``.  ``table`` / ``table_temperatures``
    default to ``power_table(temperature, max visit + 1)``."""
    t_legal = _dev(backend, legal, torch.int32)
    B, A = t_legal.shape
    t_visits = _dev(backend, visits, torch.int32)
    temps = numpy.full(B, float(temperature)) if numpy.isscalar(temperature) else temperature
    t_temps = _dev(backend, temps, torch.float64)
    if tuple(t_visits.shape) != (B, A) or tuple(t_temps.shape) != (B,):
        raise ValueError("visits [B][A] and temperature [B] must match legal")
    if table is None and not isinstance(temps, torch.Tensor):
        table, table_temperatures = power_table(temps, int(t_visits.max()) + 1 if t_visits.numel() else 1)
    keep = []
    d = _header(backend, seed, counter, B, A, streams, first_stream, keep)
    s = _lib.DrawsSelect()
    t_table, t_tt = _dev(backend, table, torch.float64), _dev(backend, table_temperatures, torch.float64)
    t_u = _dev(backend, uniforms, torch.float64)
    t_action = backend.empty((B,), torch.int64)
    s.d_legal_actions, s.d_visit_counts, s.d_temperature = backend.ptr(t_legal), backend.ptr(t_visits), backend.ptr(t_temps)
    s.d_pow_table, s.d_table_temperatures = backend.ptr(t_table), backend.ptr(t_tt)
    s.table_stride = 0 if t_table is None else int(t_table.shape[1])
    s.num_temperatures = 0 if t_table is None else int(t_table.shape[0])
    s.d_uniforms, s.d_action = backend.ptr(t_u), backend.ptr(t_action)
    backend.lib.check(backend.lib.mzx_selfplay_select_device(ctypes.byref(d), ctypes.byref(s), backend.stream()))
    return t_action
