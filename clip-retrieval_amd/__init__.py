"""MI355X-native hot path of clip-retrieval: CLIP encode + inner-product kNN behind the reference's
own seams (ClipMapper / Runner, and the faiss-Index duck type of clip_back).  See DESIGN.md.

Nothing here computes on the CPU: every product entry point goes through `lib/libclipx.so`
(HIP, gfx950) and raises `HipLibraryError` if the library or a GPU is missing.
"""

__version__ = "0.1.0"

from ._lib import HipLibraryError, ResidualStreamOverflow, load_library, library_path  # noqa: F401

# the list-ordered ids of an IVF index under the reference's names (ivf_metadata_ordering.py, clip_back.py:629-640), resolved on first
# use so that importing the package stays as light as it was
_LAZY = {"get_old_to_new_mapping": "knn", "search_to_new_ids": "knn", "load_ivf_old_to_new_mapping": "service",
         "reorder_arrow_metadata": "service",
         # the multilingual text towers of `use_mclip` (mclip.py)
         "BertArch": "mclip", "BertTextEncoder": "mclip", "WordPieceTokenizer": "mclip", "blob_from_distilbert_state_dict": "mclip",
         "blob_from_xlmr_state_dict": "mclip", "random_bert_blob": "mclip", "load_sentence_transformer": "mclip", "load_mclip": "mclip"}


def __getattr__(name):
    if name in _LAZY:
        import importlib  # pylint: disable=import-outside-toplevel

        return getattr(importlib.import_module("clip_retrieval_amd." + _LAZY[name]), name)
    raise AttributeError(f"module 'clip_retrieval_amd' has no attribute {name!r}")
