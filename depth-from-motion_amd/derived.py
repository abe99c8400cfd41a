"""State DERIVED from a module's parameters or from tensors the detector injects: packed MFMA weight fragments,
folded BatchNorm scale / shift, fp32 copies of bf16 affine parameters, device copies of host tensors, interpolation
tables.  All of it lives in a ``Derived`` cache, which makes three rules hold by construction:

1. A value is rebuilt when one of its source tensors changes: an entry is a hit only while every source is the same
   OBJECT as at build time (weak references, so a new tensor that reuses a freed ``id()`` or a freed address never
   matches a dead one) with the same version, address and device, and the non-tensor part of the key is equal.
2. It is no part of a module's identity: a cache pickles and deep-copies as a new empty cache (``torch.save(model)``,
   EMA hooks, ``mp.spawn`` arguments), and the copy rebuilds on its first forward.
3. A value is built lazily by the FIRST call that needs it, with kernels on that call's HIP stream.  Work that runs
   on two streams (DfMStereoPath: one 2-D neck for the previous frame on a side stream and for the current frame on the
   main stream; the two stacks of DfMBackbone and DfMNeck, which share process-wide caches) would let the second
   stream read what the first has not finished writing.  Every miss of a cache bumps a counter; streams.fork_join,
   the only place that forks, reads it around every step and makes the other stream wait when anything was built.
"""
import weakref

_BUILDS = [0]


def note_derived_build():
    """for the public pack functions, which launch kernels on the caller's stream with or without a cache"""
    _BUILDS[0] += 1


def derived_builds():
    return _BUILDS[0]


def _ident(t):
    return t._version, t.data_ptr(), t.device


class Derived:
    """name -> value built from ``sources`` (a tuple of tensors) and ``extra`` (hashable non-tensor key parts).
    ``capacity``: a process-wide cache clears everything before the insertion that would exceed it."""

    def __init__(self, capacity=None):
        self.capacity = capacity
        self._entries = {}

    def __reduce__(self):
        return type(self), (self.capacity,)

    def get(self, name, sources, make, extra=()):
        e = self._entries.get(name)
        if e is not None and e[2] == extra and len(e[0]) == len(sources):
            for ref, ident, t in zip(e[0], e[1], sources):
                if ref() is not t or ident != _ident(t):
                    break
            else:
                return e[3]
        value = make()
        self.put(name, sources, value, extra)
        _BUILDS[0] += 1
        return value

    def put(self, name, sources, value, extra=()):
        """what a miss of ``get`` stores (on its own: tests that inject an entry)"""
        if self.capacity is not None and len(self._entries) >= self.capacity and name not in self._entries:
            self._entries.clear()
        self._entries[name] = (tuple(weakref.ref(t) for t in sources), tuple(_ident(t) for t in sources), extra,
                               value)

    def peek(self, name):
        """the stored value, whatever became of its sources, or None (tests)"""
        e = self._entries.get(name)
        return None if e is None else e[3]


def derived(owner):
    """the cache of ``owner`` (any object with a ``__dict__``: the path's modules, an ``nn.Sequential``, whatever
    holds an injected tensor), created on first use"""
    cache = owner.__dict__.get('_derived')
    if cache is None:
        cache = owner.__dict__['_derived'] = Derived()
    return cache
