from .paged_cache import PagedCacheFull, PagedKVCache

__all__ = ["PagedKVCache", "PagedCacheFull"]
