"""What the package does with a setting its kernels do not cover, stated once.

The policy: 'warn' (default) says so once per (what, why) and runs what was there before -- torch's convolution for
an ``Mfma*`` module (``conv3d._torch_path``), the reference method or mmcv op that ``patch_reference()`` displaced for
everything else (``run_reference``) -- 'raise' (strict mode) makes it an ``MfmaPathError``, 'silent' runs it without a
word.  A module's own ``fallback_policy`` attribute (what ``integration.enable_fast_path`` sets) overrides the
process-wide mode.
"""
import warnings

_POLICY = {'mode': 'warn'}
# everything patch_reference() displaced, for the whole process: 'Class.method' -> the reference method,
# '<module>.<attr>' -> the name's previous value, 'CONV_LAYERS.<name>' / 'DCNv2' -> the registry's previous entry,
# 'modulated_deform_conv2d' -> mmcv's op
REPLACED = {}
WARNED = set()   # (what, why) already warned about


class MfmaPathError(RuntimeError):
    """strict mode: an Mfma* module was handed an input its MFMA kernel does not take"""


def set_fallback_policy(mode):
    """'warn' | 'raise' | 'silent'; returns the previous mode"""
    if mode not in ('warn', 'raise', 'silent'):
        raise ValueError(mode)
    prev, _POLICY['mode'] = _POLICY['mode'], mode
    return prev


def fallback_policy():
    return _POLICY['mode']


def module_fallback_policy(module):
    """the policy that governs ``module``: its own ``fallback_policy`` attribute (what
    ``integration.enable_fast_path`` sets on the Mfma* modules of the model it converts) or, without one,
    the process-wide mode"""
    return getattr(module, 'fallback_policy', None) or _POLICY['mode']


def warn_once(what, why, msg, stacklevel):
    """``stacklevel`` counts from the caller of this function, as ``warnings.warn`` counts from its own"""
    if (what, why) not in WARNED:
        WARNED.add((what, why))
        warnings.warn(msg, RuntimeWarning, stacklevel=stacklevel + 1)


def run_reference(owner, method, why, kernels, args, mixin=None, key=None):
    """``owner`` (a head, a module or None) met the setting ``why``, which the ``kernels`` kernels do not cover: run
    what ``patch_reference()`` displaced, under the policy that governs ``owner``.

    A method (``mixin`` given) is looked up along ``type(owner).__mro__``: the first class with an entry
    ``REPLACED['<Class>.<method>']`` -- so two patched classes each get their own original -- else the first class after
    ``mixin`` that defines ``method`` itself (``class FastHead(Mixin, RefHead)``).  A plain function is
    ``REPLACED[key]``.  Under 'raise', or with nothing to run, an ``MfmaPathError`` naming the setting; else one
    ``RuntimeWarning`` per (method or key, why), attributed to the caller of the public function that called this one,
    and the original's result."""
    if key is not None:
        original, what, running, nothing = REPLACED.get(key), key, "running mmcv's op", 'and there is no mmcv op to run'
    else:
        mro = type(owner).__mro__
        original = next((REPLACED[f'{k.__name__}.{method}'] for k in mro if f'{k.__name__}.{method}' in REPLACED), None)
        if original is None and mixin in mro:
            original = next((vars(k)[method] for k in mro[mro.index(mixin) + 1:] if method in vars(k)), None)
        what, running = f'{type(owner).__name__}.{method}', 'running the reference method'
        nothing = 'and there is no reference method to run'
    msg = (f'{what}: {why} -- not covered by the {kernels} kernels; {running}.  '
           'set_fallback_policy("raise") makes this an error.')
    policy = module_fallback_policy(owner)
    if policy == 'raise' or original is None:
        raise MfmaPathError(msg if original is not None else msg.replace(running, nothing))
    if policy != 'silent':
        warn_once(key or method, why, msg, stacklevel=3)   # past this function and the public one that called it
    return original(*args) if key is not None else original(owner, *args)
