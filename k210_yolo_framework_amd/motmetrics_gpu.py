"""motmetrics.py on the GPU (csrc/yk_mot.hip): lap, a batch of assignment problems in one launch (yk_lap_f64), held to
motmetrics.lap assignment for assignment; MotEvaluator, the three scores of packed sequences (yk_mot_eval), held to motmetrics.evaluate -
integers equal, float sums within 1e-12.  No device: an error, never a fallback."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import engine
from . import motmetrics as mm


class LapProblem(C.Structure):
    """yk_lap_problem_t"""
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('cost_offset', C.c_longlong), ('out_offset', C.c_longlong)]


def limits() -> dict:
    """The YK_LAP_* constants the library was built with (yk_lap_limit): LDS_BYTES, LDS_PER_COL, LDS_PER_ROW, MAX, MAX_LONG."""
    out = {}
    for which, name in enumerate(('LDS_BYTES', 'LDS_PER_COL', 'LDS_PER_ROW', 'MAX', 'MAX_LONG')):
        out[name] = engine.lib().yk_lap_limit(which)
        if out[name] < 0:
            engine._check(out[name], 'yk_lap_limit')
    return out


def lds_resident(rows: int, cols: int) -> bool:
    """Whether yk_lap_f64 keeps the cost matrix of a rows x cols problem in LDS (a function of the shape alone)."""
    r = engine.lib().yk_lap_lds_resident(int(rows), int(cols))
    if r < 0:
        engine._check(r, 'yk_lap_lds_resident')
    return bool(r)


def lap(costs: Sequence, stream=None) -> List[np.ndarray]:
    """costs: matrices [rows, cols], finite -> per matrix int64 [rows], the column of every row or -1, as motmetrics.lap gives it; all of
    them in one yk_lap_f64 call.  Waits for the result."""
    import torch
    engine.require_gpu()
    mats = [np.ascontiguousarray(c, np.float64) for c in costs]
    if not mats:
        return []
    table, at_c, at_o = (LapProblem * len(mats))(), 0, 0
    for k, m in enumerate(mats):
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise engine.YkError(f'lap: costs[{k}] of shape {m.shape}: expected [rows >= 1, cols >= 1]')
        if not np.isfinite(m).all():
            raise engine.YkError(f'lap: costs[{k}] has a NaN or an infinity; a forbidden pair carries 1e10')
        table[k] = LapProblem(m.shape[0], m.shape[1], at_c, at_o)
        at_c, at_o = at_c + m.size, at_o + m.shape[0]
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        d_cost = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).cuda()
        d_out = torch.empty(at_o, dtype=torch.int32, device=d_cost.device)
        engine.call('yk_lap_f64', d_cost, at_c, table, len(mats), d_out, at_o, engine._stream(stream))
        out = d_out.cpu().numpy().astype(np.int64)
    return list(np.split(out, np.cumsum([m.shape[0] for m in mats])[:-1]))


class MotShape(C.Structure):
    """yk_mot_shape_t"""
    _fields_ = [(k, C.c_int32) for k in ('n_seq', 'n_frames', 'n_gt_ids', 'n_res_ids', 'max_seq_gt_ids', 'max_seq_res_ids', 'max_seq_ids',
                                          'max_frame_gt', 'max_frame_res', 'reserved')] + \
               [(k, C.c_longlong) for k in ('n_gt_rows', 'n_res_rows', 's_cells', 'gt_cells', 'id_cells', 'max_seq_gt_cells')]


OUT_INTS, OUT_DOUBLES = 84, 80            # YK_MOT_OUT_INTS, YK_MOT_OUT_DOUBLES


class MotEvaluator:
    """add_sequence(name, gt, res) with the tables of motmetrics ([n, 6]: frame, id, left, top, width, height), then result() ->
    {'sequences': {name: scores}, 'combined': scores} with the keys of motmetrics.evaluate; every sequence added so far is scored in
    one yk_mot_eval call."""

    def __init__(self, device: int = 0):
        import torch
        engine.require_gpu()
        self.device = torch.device('cuda', int(device))
        self.seqs = []

    def add_sequence(self, name: str, gt, res) -> None:
        if any(name == s['name'] for s in self.seqs):
            raise ValueError(f'sequence {name!r} appears twice')
        gf, gi, gb, G = mm._table(name, 'ground-truth', gt)
        tf, ti, tb, T = mm._table(name, 'result', res)
        self.seqs.append(dict(name=name, gf=gf, gi=gi, gb=gb, G=G, tf=tf, ti=ti, tb=tb, T=T,
                              n_frames=int(max(gf.max(initial=0), tf.max(initial=0)))))

    def _pack(self):
        """-> (MotShape, the host tables in yk_mot_eval's order)"""
        S = self.seqs
        seq_tab = np.zeros((len(S) + 1, 5), np.int64)
        for k, s in enumerate(S):
            seq_tab[k + 1] = seq_tab[k] + [s['n_frames'], s['G'], s['T'], s['G'] * s['T'], (s['G'] + s['T']) ** 2]
        F = int(seq_tab[-1, 0])
        cat = lambda key, dt, shape=(-1,): np.concatenate([np.asarray(s[key]).reshape(shape) for s in S] or [np.zeros(0)]).astype(dt).reshape(shape)
        g_frame = np.concatenate([s['gf'] - 1 + seq_tab[k, 0] for k, s in enumerate(S)]).astype(np.int64)       # global frame of a row
        t_frame = np.concatenate([s['tf'] - 1 + seq_tab[k, 0] for k, s in enumerate(S)]).astype(np.int64)
        g_gid = np.concatenate([s['gi'] + seq_tab[k, 1] for k, s in enumerate(S)]).astype(np.int64)             # global gt id of a row
        t_gid = np.concatenate([s['ti'] + seq_tab[k, 2] for k, s in enumerate(S)]).astype(np.int64)
        frame_tab = np.zeros((F + 1, 3), np.int64)
        frame_tab[:, 0], frame_tab[:, 1] = np.searchsorted(g_frame, np.arange(F + 1)), np.searchsorted(t_frame, np.arange(F + 1))
        per_g, per_t = np.diff(frame_tab[:, 0]), np.diff(frame_tab[:, 1])
        frame_tab[1:, 2] = np.cumsum(per_g * per_t)
        order = np.argsort(g_gid, kind='stable')                                                                   # rows are in frame order already
        n_gid, n_tid = int(seq_tab[-1, 1]), int(seq_tab[-1, 2])
        gcount, tcount = np.bincount(g_gid, minlength=n_gid).astype(np.float64), np.bincount(t_gid, minlength=n_tid).astype(np.float64)
        csr_first = np.concatenate([[0], np.cumsum(gcount)]).astype(np.int32)
        sh = MotShape(n_seq=len(S), n_frames=F, n_gt_ids=n_gid, n_res_ids=n_tid, max_seq_gt_ids=max(s['G'] for s in S),
                      max_seq_res_ids=max(s['T'] for s in S), max_seq_ids=max(s['G'] + s['T'] for s in S),
                      max_frame_gt=int(per_g.max(initial=0)), max_frame_res=int(per_t.max(initial=0)), n_gt_rows=len(g_gid), n_res_rows=len(t_gid),
                      s_cells=int(frame_tab[-1, 2]), gt_cells=int(seq_tab[-1, 3]), id_cells=int(seq_tab[-1, 4]),
                      max_seq_gt_cells=max(s['G'] * s['T'] for s in S))
        tables = [cat('gb', np.float64, (-1, 4)), cat('tb', np.float64, (-1, 4)), cat('gi', np.int32), cat('ti', np.int32), frame_tab,
                  np.repeat(np.arange(len(S)), np.diff(seq_tab[:, 0])).astype(np.int32), seq_tab, csr_first, order.astype(np.int32),
                  g_frame.astype(np.int32), np.repeat(np.arange(len(S)), np.diff(seq_tab[:, 1])).astype(np.int32), gcount, tcount,
                  mm.ALPHAS - mm.EPS]
        return sh, tables

    def result(self, stream=None) -> dict:
        import torch
        if not self.seqs:
            raise engine.YkError('MotEvaluator.result: no sequence was added')
        sh, tables = self._pack()
        nbytes = C.c_size_t(0)
        engine.call('yk_mot_workspace_bytes', C.byref(sh), C.byref(nbytes))                # (refuses a sequence above the limits by name)
        with torch.cuda.device(self.device), torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream):
            dev = [torch.from_numpy(np.ascontiguousarray(t) if t.size else np.zeros(1, t.dtype)).to(self.device) for t in tables]
            ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=self.device)
            out_i = torch.empty((len(self.seqs), OUT_INTS), dtype=torch.int32, device=self.device)
            out_d = torch.zeros((len(self.seqs), OUT_DOUBLES), dtype=torch.float64, device=self.device)
            engine.call('yk_mot_eval', C.byref(sh), *dev, ws, nbytes.value, out_i, out_d, engine._stream(stream))
            oi, od = out_i.cpu().numpy().astype(np.int64), out_d.cpu().numpy()
        return self._scores(oi, od)

    def _scores(self, oi: np.ndarray, od: np.ndarray) -> dict:
        """yk_mot_eval's two outputs on the host (int64 [n_seq, OUT_INTS], float64 [n_seq, OUT_DOUBLES]) -> what result() returns"""
        per = {}
        for k, s in enumerate(self.seqs):
            i, d = oi[k], od[k]
            m = dict(HOTA_TP=i[0:19], HOTA_FN=i[19:38], HOTA_FP=i[38:57], MC=i[57:76], Loc=d[57:76])
            tp1 = np.maximum(1, m['HOTA_TP'])
            m['AssA'], m['AssRe'], m['AssPr'] = d[0:19] / tp1, d[19:38] / tp1, d[38:57] / tp1
            mm._hota_final(m)
            m.update({key: int(i[76 + n]) for n, key in enumerate(('CLR_TP', 'CLR_FN', 'CLR_FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML'))})
            m['MOTPsum'] = float(d[76])
            mm._clear_final(m)
            m['IDFN'], m['IDFP'] = int(d[77]), int(d[78])
            m['IDTP'] = int(len(s['gi'])) - m['IDFN']
            mm._identity_final(m)
            m.update(GT_IDs=s['G'], RES_IDs=s['T'], Frames=s['n_frames'])
            per[s['name']] = mm.summarise(m)
        return dict(sequences=per, combined=mm.combine(list(per.values())))
