"""A keyed cache of device tensors whose addresses a captured graph may hold.

A graph records the device pointers of its launches, so a tensor that a cache handed out while the
current stream was capturing has to live, at its address and unchanged, for as long as the graph can
be replayed. :class:`GraphCache` therefore *pins* every entry it returns under capture: a pinned entry
leaves only through :meth:`GraphCache.clear` (``invalidate_cache()``) or when the ``stale`` predicate
of a later miss names it (a parameter-version change, which invalidates the graphs as well). Entries
that were only ever used eagerly are bounded, least recently used first out, so a server that sees
many image sizes eagerly keeps a finite amount of memory; an eager launch that still reads an evicted
tensor is safe, because the caching allocator frees in stream order.

Make an entry eagerly first (a warm-up run before the capture, as for every graph): a miss under
capture is pinned too, but its tensors are then built by the capture itself.
"""
from __future__ import annotations

import threading
from collections import OrderedDict
from typing import Any, Callable, Hashable, Optional

import torch

_MISS = object()


def is_capturing() -> bool:
    """True while the current stream records a graph (False before the GPU is initialised: nothing
    can be capturing then, and the question must not initialise it)."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


class GraphCache:
    def __init__(self, bound: int, capturing: Optional[Callable[[], bool]] = None):
        if bound < 1:
            raise ValueError("GraphCache: room for at least one unpinned entry")
        self.bound = bound
        #: the predicate that pins; None means this module's :func:`is_capturing`, looked up per call
        self.capturing = capturing
        self._d: "OrderedDict[Hashable, Any]" = OrderedDict()
        self._pinned: set = set()
        self._lock = threading.Lock()

    def get(self, key: Hashable, make: Callable[[], Any], stale: Optional[Callable[[Hashable], bool]] = None) -> Any:
        """The entry of ``key``, made by ``make()`` on a miss. A miss first drops every entry, pinned
        or not, whose key ``stale`` names, then the least recently used unpinned entries beyond
        ``bound - 1``."""
        pin = (self.capturing or is_capturing)()
        with self._lock:
            hit = self._d.get(key, _MISS)
            if hit is not _MISS:
                self._touch(key, pin)
                return hit
        value = make()
        with self._lock:
            hit = self._d.get(key, _MISS)
            if hit is not _MISS:    # another thread made it meanwhile: one object per key
                self._touch(key, pin)
                return hit
            if stale is not None:
                for k in [k for k in self._d if stale(k)]:
                    del self._d[k]
                    self._pinned.discard(k)
            while len(self._d) - len(self._pinned) >= self.bound:
                del self._d[next(k for k in self._d if k not in self._pinned)]
            self._d[key] = value
            if pin:
                self._pinned.add(key)
        return value

    def _touch(self, key: Hashable, pin: bool) -> None:
        if pin:
            self._pinned.add(key)
        elif key not in self._pinned:
            self._d.move_to_end(key)

    def clear(self) -> None:
        """Drop every entry, the pinned ones included: graphs that hold them must be captured again."""
        with self._lock:
            self._d.clear()
            self._pinned.clear()

    def pinned(self, key: Hashable) -> bool:
        return key in self._pinned

    def unpinned(self) -> int:
        return len(self._d) - len(self._pinned)

    def __len__(self) -> int:
        return len(self._d)

    def __contains__(self, key: Hashable) -> bool:
        return key in self._d

    def __deepcopy__(self, memo) -> "GraphCache":
        # a copied model owns other parameters: it starts with an empty cache of its own
        return GraphCache(self.bound, self.capturing)
