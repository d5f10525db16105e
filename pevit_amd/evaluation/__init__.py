"""Host-side mirror of ``vision_benchmark.evaluation`` for the PEFT fine-tune path.

Same importable names and call signatures as the reference's Python modules; the vision tower,
head, loss and optimiser execute in ``libpevit_hip.so``.  Dataset download/manifest code, the BPE
vocabulary and the knowledge-augmented prompt sources of the reference are not part of this path.
"""
from .dataloader import construct_dataloader  # noqa: E402,F401
from .feature import extract_features, extract_text_features, zeroshot_scores  # noqa: E402,F401
from .clip_zeroshot_evaluator import clip_zeroshot_evaluator  # noqa: E402,F401
