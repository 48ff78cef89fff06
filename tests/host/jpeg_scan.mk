# make -C tests/host -f jpeg_scan.mk jpeg_scan_test
# The parser and the scan decoder of sfm_jpeg.hpp with a coefficient sink (what the device decoder's host side calls), under
# AddressSanitizer + UBSan like jpeg_test_asan of the Makefile beside this file; the header alone, no library.
jpeg_scan_test: jpeg_scan_test.cpp ../../sfm_opencv_amd/host/sfm_jpeg.hpp
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -I../../sfm_opencv_amd/host -o $@ jpeg_scan_test.cpp
