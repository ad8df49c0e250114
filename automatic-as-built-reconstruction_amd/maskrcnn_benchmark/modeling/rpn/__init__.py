"""The first stage: anchors, the RPN head and RPNModule (reference: maskrcnn_benchmark/modeling/rpn/)."""
