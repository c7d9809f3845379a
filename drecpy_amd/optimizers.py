"""Optimizer objects for `fit(optimizer=...)` and `RecommenderABC._register_optimizer` (recommender_abc.py:153-156, 284).

The reference accepts any tf.keras optimizer.  The engine's update rules are hand-written kernels, so the accepted set is:

    None / 'adam' / Adam(...)          Keras Adam (default: learning_rate of fit(), beta_1 .9, beta_2 .999, epsilon 1e-7)
    'adagrad' / Adagrad(...)           Keras Adagrad (initial_accumulator_value .1, epsilon 1e-7)
    'sgd' / SGD(...)                   Keras SGD: plain (no slot), momentum, Nesterov momentum
    'rmsprop' / RMSprop(...)           Keras RMSprop (rho .9, epsilon 1e-7), with or without momentum; centered=True is refused
    'rowwise_adagrad'                  one accumulator per table row (engine extension)            — CDAE mode='sampled' only

The rules' arithmetic is the table of include/drx.h (DrxOptRule), fp32 in TF's order of operations.  Adam, Adagrad, SGD and RMSprop
drive every dense step (`apply_gradients` here; the fused steps take the rule through `rule()`); none but Adam has a bias correction,
so their step size is the learning rate itself.  Anything else — a TensorFlow optimizer object, Adadelta / Adamax / Nadam / Ftrl,
`amsgrad`, `clipnorm` / `clipvalue`, a learning-rate schedule — is rejected with the accepted list in the message.

`apply_gradients` is the reference's call (one call = one `iterations` tick shared by all pairs of the call) running
`drx_opt_dense` on the device: what `RecommenderABC._update_weights` uses for variables a model updates outside a fused
step.  A rule's slots (`N_SLOTS`: 0 for plain SGD, 1, or 2 for Adam and RMSprop with momentum) are the only arrays it allocates.
"""
import numpy as np


KINDS = {'adam': 0, 'adagrad': 1, 'rowwise_adagrad': 2, 'sgd': 3, 'momentum': 4, 'nesterov': 5, 'rmsprop': 6, 'rmsprop_momentum': 7}   # DRX_OPT_*
N_SLOTS = {'adam': 2, 'adagrad': 1, 'rowwise_adagrad': 1, 'sgd': 0, 'momentum': 1, 'nesterov': 1, 'rmsprop': 1, 'rmsprop_momentum': 2}


def _number(name, value):
    """Hyper-parameters are whatever float() takes: a schedule object or a callable cannot drive the kernels."""
    if not callable(value):
        try:
            return float(value)
        except (TypeError, ValueError):
            pass
    raise Exception(f'{name}={value!r}: the update kernels take a constant number (learning-rate schedules and callables are not supported)')


def _no_extras(cls, kwds):
    if kwds:
        raise Exception(f'{cls}: unsupported argument(s) {sorted(kwds)} — amsgrad, clipnorm / clipvalue / global_clipnorm, decay and the like '
                        f'have no kernel here; accepted values are {ACCEPTED}')


class _Dense:
    """What the dense rules share: the call counter, the slots of every variable and apply_gradients over drx_opt_dense."""
    slot_init = 0.0

    def _init_state(self):
        self.iterations = 0
        self._slots = {}              # id(Variable) -> (weak reference, s1, s2);  ('view', storage, offset, shape, strides) -> (storage, s1, s2)

    def reset(self):
        """A fresh fit(): the call counter and the slots start over (RecommenderABC.fit registers the optimizer anew)."""
        self._init_state()

    @property
    def n_slots(self):
        return N_SLOTS[self.kind]

    def _new_slots(self, p):
        import torch
        return tuple(torch.full_like(p, self.slot_init) if i < self.n_slots else None for i in range(2))

    def _moments(self, owner, p):
        """(s1, s2) of one variable (Adam: m, v), None for a slot the rule does not have.  A Variable OBJECT is keyed by identity (weak
        reference: a new object at a recycled id starts afresh).  A bare tensor is keyed by WHAT IT VIEWS — storage, offset, shape,
        strides: a layer / model handle hands out
        fresh view objects of the same memory on every `trainable_weights` read (trainables._Handle), and those must find their
        moments again (keyed by id() they silently restarted from zero every step).  The entry holds the storage, so
        the memory cannot be freed and handed to another tensor while its moments exist (reset() drops them with a new fit())."""
        import weakref
        import torch
        if torch.is_tensor(owner):
            st = owner.untyped_storage()
            key = ('view', st._cdata, owner.storage_offset(), tuple(owner.shape), tuple(owner.stride()))
            ent = self._slots.get(key)
            if ent is None:
                ent = self._slots[key] = (st,) + self._new_slots(p)
            return ent[1], ent[2]
        ent = self._slots.get(id(owner))
        if ent is not None and (ent[0]() is not owner or any(s is not None and (s.shape != p.shape or s.device != p.device) for s in ent[1:])):
            ent = None                  # the id was recycled by another object, or the variable was rebound to another shape / device
        if ent is None:
            try:
                ref = weakref.ref(owner)
            except TypeError:
                ref = (lambda o: (lambda: o))(owner)
            ent = self._slots[id(owner)] = (ref,) + self._new_slots(p)
            for k in [k for k, e in self._slots.items() if not isinstance(k, tuple) and e[0]() is None]:
                del self._slots[k]
        return ent[1], ent[2]

    def rule(self, step_size=None):
        """The _lib.OptRule (include/drx.h DrxOptRule) of this optimizer; step_size: Adam's lr_t of the call (default: the learning rate)."""
        from . import _lib
        mu, mu2 = self._mus()
        return _lib.OptRule(KINDS[self.kind], self.learning_rate if step_size is None else step_size, mu, mu2, getattr(self, 'epsilon', 0.0))

    def _step_size(self):
        return self.learning_rate

    def apply_gradients(self, grads_and_vars):
        import ctypes as C
        import torch
        from . import _lib
        self.iterations += 1
        rule = self.rule(self._step_size())
        for g, var in grads_and_vars:
            p = getattr(var, 'tensor', var)
            if not (torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise Exception(f'apply_gradients needs contiguous fp32 device arrays (drecpy_amd Variable or tensor), got {type(var).__name__}')
            g = torch.as_tensor(g, dtype=torch.float32, device=p.device).reshape(p.shape).contiguous()
            live = [t for t in self._moments(var, p) if t is not None]
            if p.data_ptr() % 16 or p.numel() % 4:                       # drx_opt_dense moves float4: pad odd-sized variables
                n4 = (p.numel() + 3) // 4 * 4
                buf = torch.zeros(2 + len(live), n4, dtype=torch.float32, device=p.device)
                for r, t in enumerate([p] + live + [g]):
                    buf[r, :p.numel()] = t.reshape(-1)
                rows = [buf[1 + i] if i < len(live) else None for i in range(2)]
                _lib.check(_lib.lib().drx_opt_dense(_lib.ptr(buf[0]), _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(buf[1 + len(live)]), n4, C.byref(rule),
                                                    0.0, _lib.stream_ptr(p.device)), 'drx_opt_dense')
                for r, t in enumerate([p] + live):
                    t.reshape(-1).copy_(buf[r, :p.numel()])
            else:
                rows = live + [None] * (2 - len(live))
                _lib.check(_lib.lib().drx_opt_dense(_lib.ptr(p), _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(g), p.numel(), C.byref(rule), 0.0,
                                                    _lib.stream_ptr(p.device)), 'drx_opt_dense')


class Adam(_Dense):
    kind = 'adam'

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, **kwds):
        if amsgrad:
            raise Exception(f'Adam(amsgrad=True) has no kernel here; accepted values are {ACCEPTED}')
        _no_extras('Adam', kwds)
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = (_number(n, v) for n, v in (
            ('learning_rate', learning_rate), ('beta_1', beta_1), ('beta_2', beta_2), ('epsilon', epsilon)))
        self._init_state()

    def _mus(self):
        return self.beta_1, self.beta_2

    def lr_t(self, t):
        """Keras-Adam step size for the 1-based call counter t, in fp32 like optimizer_v2/adam.py."""
        f = np.float32
        return float(f(self.learning_rate) * np.sqrt(f(1.0) - np.power(f(self.beta_2), f(t))) / (f(1.0) - np.power(f(self.beta_1), f(t))))

    def _step_size(self):
        return self.lr_t(self.iterations)


class Adagrad(_Dense):
    kind = 'adagrad'

    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, **kwds):
        _no_extras(type(self).__name__, kwds)
        self.learning_rate, self.initial_accumulator_value, self.epsilon = (_number(n, v) for n, v in (
            ('learning_rate', learning_rate), ('initial_accumulator_value', initial_accumulator_value), ('epsilon', epsilon)))
        self._init_state()

    @property
    def slot_init(self):
        return self.initial_accumulator_value

    def _mus(self):
        return 0.0, 0.0


class RowwiseAdagrad(Adagrad):
    kind = 'rowwise_adagrad'

    def apply_gradients(self, grads_and_vars):
        raise Exception('rowwise_adagrad is applied only inside the fused sparse CDAE step (mode="sampled"); use another rule for _update_weights')


class SGD(_Dense):
    """Keras SGD.  kind: 'sgd' (momentum == 0: no slot), 'momentum', 'nesterov'."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, **kwds):
        _no_extras('SGD', kwds)
        self.learning_rate, self.momentum, self.nesterov = _number('learning_rate', learning_rate), _number('momentum', momentum), bool(nesterov)
        if not 0.0 <= self.momentum <= 1.0:
            raise Exception(f'SGD(momentum={momentum!r}): must lie in [0, 1]')
        self._init_state()

    @property
    def kind(self):
        # (Keras: nesterov without momentum is plain SGD — its dense apply takes the momentum branch only when momentum > 0)
        return 'sgd' if self.momentum == 0.0 else ('nesterov' if self.nesterov else 'momentum')

    def _mus(self):
        return self.momentum, 0.0


class RMSprop(_Dense):
    """Keras RMSprop.  kind: 'rmsprop' (momentum == 0: one slot, epsilon outside the root), 'rmsprop_momentum' (two, epsilon inside)."""

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, **kwds):
        if centered:
            raise Exception(f'RMSprop(centered=True) has no kernel here; accepted values are {ACCEPTED}')
        _no_extras('RMSprop', kwds)
        self.learning_rate, self.rho, self.momentum, self.epsilon = (_number(n, v) for n, v in (
            ('learning_rate', learning_rate), ('rho', rho), ('momentum', momentum), ('epsilon', epsilon)))
        if not 0.0 <= self.momentum <= 1.0:
            raise Exception(f'RMSprop(momentum={momentum!r}): must lie in [0, 1]')
        self.centered = False
        self._init_state()

    @property
    def kind(self):
        return 'rmsprop' if self.momentum == 0.0 else 'rmsprop_momentum'

    def _mus(self):
        return self.momentum, self.rho


ACCEPTED = ("None, 'adam', 'adagrad', 'sgd', 'rmsprop', 'rowwise_adagrad', drecpy_amd.optimizers.Adam(...), drecpy_amd.optimizers.Adagrad(...), "
            "drecpy_amd.optimizers.SGD(...), drecpy_amd.optimizers.RMSprop(...)")


def resolve(optimizer, learning_rate):
    """fit()'s `optimizer=` argument -> one of the objects above; raises for anything the kernels do not implement."""
    if optimizer is None or optimizer == 'adam':
        return Adam(learning_rate)
    if optimizer == 'adagrad':
        return Adagrad(learning_rate)
    if optimizer == 'rowwise_adagrad':
        return RowwiseAdagrad(learning_rate)
    if optimizer == 'sgd':
        return SGD(learning_rate)
    if optimizer == 'rmsprop':
        return RMSprop(learning_rate)
    if isinstance(optimizer, _Dense):
        return optimizer
    raise Exception(f'Unsupported optimizer {optimizer!r}: the update rules are hand-written HIP kernels, accepted values are {ACCEPTED}. '
                    f'(The reference takes any tf.keras optimizer, recommender_abc.py:155-156; TensorFlow objects cannot drive this engine.)')
