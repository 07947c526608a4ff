"""One rule for state derived from the weights: it follows them.

A model that has decoded holds copies and captures of its weights: the W4K buffers of the 4-bit Linears (``_packed``, ``_codes``),
the concatenated SwiGLU pair of the LLM.int8 ones (``_pair``), the stream engine's E4 / E16 / E8 images (``model._engine_images``)
and the captured decode steps (``model._decode_sessions``, ``model._chat_sessions``), whose launches carry raw device pointers.
All of it is valid for ONE state of the weights, named by two counters:

  * every quantised Linear carries ``image_epoch``, a draw from one process-wide counter (``next_epoch``): it moves on in the
    module's ``_load_from_state_dict`` / ``_apply`` / ``_quantize_weight`` / ``pack_weight`` and when a reference buffer is assigned;
  * the model carries a counter of its own for what no module sees: ``load_state_dict`` and ``_apply`` on the model,
    ``checkpoint.stream_load``, ``synth.build_synthetic_model`` and the explicit ``weights_changed(model)``.

``weights_generation(model)`` is their sum.  The epochs are unique and growing, so the sum grows with every change, also when a
Linear is replaced by a newly built one.  Sessions record the generation they were built under and are stale under any other;
engine images are keyed by it.  What nothing can see is an edit through ``.data`` (torch does not move ``_version`` for it):
call ``weights_changed(model)`` after one.
"""
import itertools

import torch

from ._hip import ParrotHipError

_epochs = itertools.count(1)


def next_epoch() -> int:
    """A value no ``image_epoch`` of this process has held, larger than all of them."""
    return next(_epochs)


def weights_generation(model: torch.nn.Module) -> int:
    """The state of the model's weights as one int: equal as long as nothing that is allowed to change weights has run."""
    return model.__dict__.get("_weights_gen", 0) + sum(getattr(m, "image_epoch", 0) for m in model.modules())


def image_stamp(model: torch.nn.Module, lin: torch.nn.Module, partner=None, k0: int = 0, k1=None, generation=None) -> tuple:
    """Key of a stream-engine image: the Linear (and its SwiGLU partner), the K-chunk and the state of the weights it was built
    from.  ``generation``: ``weights_generation(model)`` when the caller has it at hand."""
    def one(m):
        return None if m is None else (id(m), getattr(m, "image_epoch", 0))

    k1 = lin.in_features if k1 is None else k1
    return (one(lin), one(partner), k0, k1, weights_generation(model) if generation is None else generation)


def weights_changed(model: torch.nn.Module) -> None:
    """Tell ``model`` that its weights are no longer what its derived state was built from: after an edit through ``.data`` (a
    merge, an optimiser step), which nothing else can see.  Drops the captured decode steps, the engine images and every
    module's kernel-layout copy; they are rebuilt from the current weights on next use.  Loading and moving the model call this
    themselves."""
    if not isinstance(model, torch.nn.Module):
        raise ParrotHipError("weights_changed() takes the model (a torch.nn.Module)")
    d = model.__dict__
    d["_weights_gen"] = d.get("_weights_gen", 0) + 1
    for name in ("_decode_sessions", "_chat_sessions", "_engine_images"):
        d.pop(name, None)
    if hasattr(model, "adapter_kv_caches"):
        model.adapter_kv_caches.clear()  # (the adapter prefix K/V are computed from the weights: adapter.py)
    for m in model.modules():
        if not hasattr(m, "image_epoch"):
            continue
        restore = getattr(m, "restore_reference", None)
        if restore is not None:
            restore()  # (an int4 Linear whose W4K buffer is its only image: the reference buffers come back first)
        for attr in ("_packed", "_pair", "_codes"):
            if attr in m.__dict__:
                m.__dict__[attr] = None
        m.image_epoch = next_epoch()
