"""Combine several trained models: aggregated posteriors and the latent mutual information of a pair (reference:
module/aggregation.py; the pairwise step of module/cascad.py; results/aggregation.py:321-374).

The public names of the reference's module - TEMPS, NAN_TEMPS, log_mean_exp, posterior, joint_posterior, mean_posterior,
voting_posterior, compute_latent_mutual_info, latent_mutual_info - with the same arguments and the same returned
dictionaries {temperature: tensor}.  Underneath, three kernels of csrc/aggregate.hip (ops.class_posterior,
ops.latent_mutual_info, ops.aggregate_scores): log p(z | c) for every class comes from ONE pass over the draws instead of
a (C, L, N, K) expansion of z, the pairwise mean of logs is taken without the two (C, L1, L0, N) tensors and their product,
every aggregated posterior is one launch for all of its temperatures.  There is no CPU path: CPU tensors raise
jvae_hip.JvaeHipError.

Kept from the reference: `posterior()` applies its soft-max over axis 0 whatever `axis` says; a temperature of NAN_TEMPS
returns the logits; `latent_mutual_info(m1, m2, x, y, temps=[1])` returns ({T: Im}, y_) with y_ = logp.mean(1).argmax(0)
of the first model.

Deliberate differences:
  * Im comes back as a plain (N,) tensor (the reference returns a named tensor whose callers strip the names at once).
  * `latent_mutual_info` accepts models whose latent_sampling or latent_dim differ: the reference's version aliases the two
    models' z and only runs when their shapes match; the composition module/cascad.py uses (compute_latent_mutual_info on
    each model's own posteriors) has no such limit, gives the same numbers, and is what runs here.
  * `latent_mutual_info` draws the latent noise itself unless `epsilon=(eps1, eps2)` ((L + 1, N, K) each) is given.
  * `voting_posterior` takes an optional `num_classes`; the default is the largest label over ALL voters + 1 (one value read
    from the device).  The reference infers the width per voter and raises when the voters disagree on it.  A vote outside
    [0, num_classes) raises JvaeHipError here and in `ensemble(..., 'vote')` (the launch's status word is read back).
  * `mean_of_posteriors` is a new name for the `mean~` aggregation the reference has only inside its results script.
  * `ensemble(scores, agg, temps)` is new: the per-combination quantities of results/aggregation.py:321-374 from the
    recorder tensors of several models.
  * Only Gaussian priors are built for the class posteriors of `latent_mutual_info`; the tilted and uniform priors raise
    NotImplementedError by name (their log_density stays on the existing path).
  * At most 128 classes, 8 models and 16 temperatures per call (the kernels' limits): beyond them JvaeHipError.

Not rebuilt, they stay in the reference: the command-line block of module/aggregation.py and the command-line, pandas and
TeX parts of results/aggregation.py - host-side bookkeeping around these functions.
"""
import torch

from jvae_hip import ops

TEMPS = [None, 1, 5]
NAN_TEMPS = [None, -1, 0]


def _rows(t):
    """(C, ...) -> ((C, M) view or copy, the trailing shape)."""
    return t.reshape(t.shape[0], -1), tuple(t.shape[1:])


def _slots(post, temps, tail):
    return {t: post[i].view(post.shape[1], *tail) for i, t in enumerate(temps)}


def _is_nan_temp(t):
    return any(t is n or (t is not None and n is not None and t == n) for n in NAN_TEMPS)


def _own_status(t):
    """A cleared status word for one launch on the device of t (the shared per-device word stays untouched)."""
    ops.L.ptr(t)                       # raises on a CPU tensor
    return torch.zeros(1, dtype=torch.int32, device=t.device)


def log_mean_exp(*tensors, normalize=False):
    """log of the mean of exp over the given tensors (all of one shape), max-shifted: one launch."""
    flat = [t.reshape(1, -1) for t in tensors]
    _, a, _, _ = ops.aggregate_scores(flat, 'mean', post=False, a=True)
    out = a.view(tensors[0].shape)
    return out.squeeze(0) if out.dim() and out.shape[0] == 1 else out


def posterior(logits, axis=0, temps=TEMPS):
    """{T: softmax over axis 0 of logits / T} (whatever `axis` says, as in the reference); T in NAN_TEMPS: the logits."""
    rows, tail = _rows(logits)
    post, _, _, _ = ops.aggregate_scores([rows], 'joint', factors=1., temps=temps)
    return _slots(post, list(temps), tail)


def joint_posterior(*zdist, axis=0, temps=TEMPS):
    """posterior(-(sum of the models' zdist) / 2): the models' latent spaces side by side."""
    rows, tail = zip(*[_rows(z) for z in zdist])
    post, _, _, _ = ops.aggregate_scores(rows, 'joint', factors=-0.5, temps=temps)
    return _slots(post, list(temps), tail[0])


def mean_posterior(*p_x_y, axis=0, temps=TEMPS):
    """posterior(log_mean_exp of the models' log p(x | y)) (their iws rows)."""
    rows, tail = zip(*[_rows(p) for p in p_x_y])
    post, _, _, _ = ops.aggregate_scores(rows, 'mean', temps=temps)
    return _slots(post, list(temps), tail[0])


def mean_of_posteriors(*logits, axis=0, temps=TEMPS, factor=1.):
    """The mean over the models of posterior(factor * logits) - the `mean~` aggregation (results/aggregation.py:330-334 applies
    it to the kl rows with factor = -1).  T in NAN_TEMPS: the mean of the scaled logits."""
    rows, tail = zip(*[_rows(p) for p in logits])
    post, _, _, _ = ops.aggregate_scores(rows, 'mean_soft', factors=float(factor), temps=temps)
    return _slots(post, list(temps), tail[0])


def voting_posterior(*y, temps=[None], num_classes=None):
    """{T: share of the voters that chose each class} (C, N), the same tensor for every T.  y: (N,) int64 predictions.  A vote
    outside [0, num_classes) raises JvaeHipError: the launch's own status word is read back here (one synchronisation)."""
    if num_classes is None:
        for v in y:
            ops.L.ptr(v)               # raises on a CPU tensor before anything is read
        num_classes = int(torch.stack([v.max() for v in y]).max()) + 1
    status = _own_status(y[0])
    _, a, _, _ = ops.aggregate_scores(y, 'vote', post=False, a=True, num_classes=num_classes, status=status)
    ops.wim_check_status(status)
    return {t: a for t in temps}


def compute_latent_mutual_info(pyz1, pyz2, sampling1=None, sampling2=None):
    """pyz1 (C, L1, N), pyz2 (C, L2, N): p(y | z) of each model's own draws -> Im (N,), the mean over the L1 x L2 draw pairs
    of log sum_y pyz1 pyz2.  sampling1 / sampling2 are the L's (read from the shapes; checked when given)."""
    if pyz1.dim() != 3 or pyz2.dim() != 3:
        raise ValueError('(C, L, N) posteriors expected, got {} and {}'.format(tuple(pyz1.shape), tuple(pyz2.shape)))
    for s, p in ((sampling1, pyz1), (sampling2, pyz2)):
        if s is not None and s != p.shape[1]:
            raise ValueError('sampling {} but {} draws given'.format(s, p.shape[1]))
    return ops.latent_mutual_info(pyz1.unsqueeze(0), pyz2.unsqueeze(0))[0]


def class_posteriors(prior, z, temps=(1,), logp=True):
    """(logp (C, L, N) or None, P (nT, C, L, N)) of the draws z (L, N, K) under every component of a conditional Gaussian prior."""
    kind = getattr(prior, 'distribution', type(prior).__name__)
    if kind != 'gaussian':
        raise NotImplementedError('class posteriors of latent draws are built for the gaussian prior, not for the {} '
                                  'prior'.format(kind))
    if not prior.conditional:
        raise ValueError('a prior with one component per class is needed')
    return ops.class_posterior(z, prior.mean.detach(), prior._var_parameter.detach(), prior.log_det_per_class().detach(),
                               var_dim=prior.var_dim, temps=temps, logp=logp)


def latent_mutual_info(m1, m2, x, y, temps=[1], epsilon=None):
    """({T: Im (N,)}, y_) for the images x (N, ...): each model encodes x and draws its own z; Im[n] is the mean over the pairs
    of draws (one of each model) of log sum_c p1(c | z1) p2(c | z2), with p(c | z) = softmax_c(log p(z | c) / T); y_ (N,) is
    the first model's prediction, argmax_c of its mean log p(z | c).  y is not used (as in the reference).  epsilon: the pair
    of the models' (L + 1, N, K) reparameterisation noises."""
    assert m1.is_cvae and m2.is_cvae
    assert m1.input_shape == m2.input_shape
    assert m1.num_labels == m2.num_labels
    temps = list(temps)
    if any(_is_nan_temp(t) for t in temps):
        raise ValueError('latent_mutual_info needs proper temperatures, got {}'.format(temps))
    eps = (None, None) if epsilon is None else epsilon
    pyz, y_ = [], None
    with torch.no_grad():
        for i, m in enumerate((m1, m2)):
            z = m.forward(x, epsilon=eps[i])[-1][1:]
            z = z.reshape(z.shape[0], -1, z.shape[-1])
            logp, P = class_posteriors(m.encoder.prior, z, temps, logp=i == 0)
            pyz.append(P)
            if i == 0:
                _, _, _, y_ = ops.aggregate_scores([logp.mean(1)], 'joint', factors=1., post=False, argmax=True)
        Im = ops.latent_mutual_info(pyz[0], pyz[1])
    return {t: Im[i] for i, t in enumerate(temps)}, y_


_ENSEMBLES = {'mean': ('iws', 'mean', 1.), 'joint': ('zdist', 'joint', -0.5), 'mean~': ('kl', 'mean_soft', -1.)}


def ensemble(scores, agg, temps=TEMPS):
    """What results/aggregation.py:321-374 computes for one combination of models.  scores: the recorder tensors of the models,
    {'iws' | 'zdist' | 'kl': [(C, N), ...]} ('vote': {'y': [(N,) int64, ...]} and optionally 'num_classes'); agg: 'mean'
    (mean_posterior of iws), 'joint' (joint_posterior of zdist), 'mean~' (mean_of_posteriors of -kl) or 'vote'
    (voting_posterior) -> {'p_y_x': {T: (C, N)}, 'y': (N,) the argmax of p_y_x[temps[0]], lowest class first,
    'max_p_y_x': its maximum[, 'log_p_x_y': log_mean_exp(iws).max(0) for 'mean']}.  One launch ('mean' with a proper first
    temperature: two)."""
    temps = list(temps)
    if agg == 'vote':
        votes = scores['y']
        C = scores.get('num_classes')
        if C is None:
            for v in votes:
                ops.L.ptr(v)
            C = int(torch.stack([v.max() for v in votes]).max()) + 1
        status = _own_status(votes[0])
        post, _, top, arg = ops.aggregate_scores(votes, 'vote', temps=temps, amax=True, argmax=True, slot=0, num_classes=C,
                                                 status=status)
        ops.wim_check_status(status)               # a vote outside [0, C) raises here, not in someone else's check
        return {'p_y_x': {t: post[0] for t in temps}, 'y': arg, 'max_p_y_x': top}
    if agg not in _ENSEMBLES:
        raise ValueError('aggregation {!r} unknown (one of mean, joint, mean~, vote)'.format(agg))
    key, mode, f = _ENSEMBLES[agg]
    # with the aggregated row written out the kernel computes it once and reads it back for every temperature
    post, a, top, arg = ops.aggregate_scores(scores[key], mode, factors=f, temps=temps, a=mode != 'mean_soft', amax=True, argmax=True,
                                             slot=0)
    out = {'p_y_x': {t: post[i] for i, t in enumerate(temps)}, 'y': arg, 'max_p_y_x': top}
    if agg == 'mean':
        if _is_nan_temp(temps[0]):                 # slot 0 is the aggregated row itself: its maximum is log_p_x_y
            out['log_p_x_y'] = top
        else:
            _, _, out['log_p_x_y'], _ = ops.aggregate_scores([a], 'joint', factors=1., post=False, amax=True)
    return out
